"""Time in the three reassemblers, CPU side: the timed models
(tests/defrag_time_model.py, tests/tcpasm_time_model.py) pinned on the
reference's own tests and comments, the conditions the GPU tests rely on
checked on the very inputs they use (tests/defragtimecases.py,
tests/tcpasmtimecases.py), the free-list rule, and the C side of the new entry
points: declared, exported, listed, and laid out as gopacket_amd/_lib.py says.
The device paths are tests/test_defrag_time_gpu.py and
tests/test_tcpasm_time_gpu.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

import defrag6_model as M6
import defrag_model as M4
import defragtimecases as TC
import flowcases
import tcpasm_model as MT
import tcpasm_time_model as TTM
import tcpasmcases
import tcpasmtimecases as TT
from gopacket_amd import _lib
from oracle import flows_oracle as FO
from test_defrag_cpu import SEQUENCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpk_defrag_batch_timed", "gpk_defrag6_batch_timed", "gpk_tcpasm_batch_timed")


def test_reference_discard_pins():
    """TestDefragDiscard (ip4defrag/defrag_test.go:223-233): two first fragments
    of two pings, then DiscardOlderThan(time.Now()) returns 2. And :63-66: after
    the datagram of TestDefragPingMultipleFrags completed, it returns 0."""
    frames, _ = flowcases.defrag_frames()
    pk = [frames["testPing1Frag1"], frames["testPing2Frag1"]]
    r = TC.model4(pk, [TC.ts(0), TC.ts(1)], [(2, TC.ts(2))])
    assert r["discards"] == [(2, 2)] and r["pending"] == [] and r["verdict"] == [M4.HELD, M4.HELD]
    order, expect = SEQUENCES["TestDefragPingMultipleFrags"]
    pk = [frames[k] for k in order]
    r = TC.model4(pk, [TC.ts(i) for i in range(len(pk))], [(len(pk), TC.ts(len(pk)))])
    assert [v >= 0 for v in r["verdict"]] == expect
    assert r["discards"] == [(0, 0)] and r["pending"] == []


def test_conditions_ipv4():
    pk, seen, t, pending, dropped = TC.conditions4()
    r = TC.model4(pk, seen, [(len(pk), t)])
    assert r["pending"] == pending and r["discards"] == [dropped]
    v = r["verdict"]
    assert v[4] == M4.HELD and v[12] == M4.EHOLE and v[14] == FO.FRAG_TOO_SMALL and v[16] == 0 and v[19] == 1
    assert v[20] < 0 and v[20] not in (M4.HELD, M4.EHOLE)
    ps = dict(zip(r["pending"], r["pending_seen"]))
    assert ps[0] == ps[5] == TC.ts(TC.YOUNG) and ps[8] == t and ps[10] == ps[12] == TC.ts(TC.YOUNG)
    # without the discard everything that was counted is pending, the duplicate and the small fragment are not
    r0 = TC.model4(pk, seen)
    assert r0["pending"] == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17] and r0["discards"] == []
    # each key is kept by its late stamp alone: with that stamp old it goes
    for late, gone in ((5, [0, 5]), (7, [6, 7]), (12, [10, 11, 12]), (17, [17])):
        s2 = list(seen)
        s2[late] = TC.ts(TC.OLD)
        r2 = TC.model4(pk, s2, [(len(pk), t)])
        assert r2["pending"] == [i for i in pending if i not in gone], late
    # the duplicate did NOT restamp: a stamp would have kept key C
    assert 3 not in r["pending"] and seen[4] >= t


def test_conditions_ipv6():
    pk, seen, t, pending, dropped = TC.conditions6()
    r = TC.model6(pk, seen, [(len(pk), t)])
    assert r["pending"] == pending and r["discards"] == [dropped]
    assert r["verdict"] == [M6.HELD] * 6 + [0, M6.HELD, 1, M6.HELD, M6.HELD, M6.NONE]
    ps = dict(zip(r["pending"], r["pending_seen"]))
    assert ps[0] == TC.ts(TC.YOUNG) and ps[3] == t and ps[9] == ps[10] == TC.ts(TC.YOUNG)
    r0 = TC.model6(pk, seen)
    assert r0["pending"] == [0, 2, 3, 4, 5, 6, 7, 8, 9, 10] and r0["discards"] == []
    # the duplicate DID restamp: with its stamp old the key goes, though the duplicate was never listed
    for late, gone in ((1, [0]), (6, [5, 6]), (10, [9, 10])):
        s2 = list(seen)
        s2[late] = TC.ts(TC.OLD)
        r2 = TC.model6(pk, s2, [(len(pk), t)])
        assert r2["pending"] == [i for i in pending if i not in gone], late


def test_streams_exercise_the_discards():
    """The streaming sequences the GPU tests cut at every position: every
    discard finds something, none empties the state, datagrams complete before
    and after, and IPv6 key 900 survives its second discard only through the
    stamp of an ignored duplicate."""
    pk, seen, ops = TC.stream4()
    r = TC.model4(pk, seen, ops)
    assert 55 <= len(pk) <= 75
    assert all(k > 0 for k, _ in r["discards"]) and r["pending"] and len(r["datagrams"]) >= 4
    assert M4.HELD in r["verdict"] and any(v < 0 and v > -16 for v in r["verdict"])
    lone = 30
    assert lone in TC.model4(pk, seen, ops[:1])["pending"] and lone not in r["pending"]

    pk, seen, ops = TC.stream6()
    r = TC.model6(pk, seen, ops)
    assert 55 <= len(pk) <= 75
    assert all(k > 0 for k, _ in r["discards"]) and r["pending"] and len(r["datagrams"]) >= 4
    assert pk[12] == pk[37]
    upto = TC.model6(pk[:41], seen[:41], [(p, t) for p, t in ops if p <= 41])
    assert 12 in upto["pending"] and 37 not in upto["pending"]
    assert upto["pending_seen"][upto["pending"].index(12)] == seen[37]
    s2 = list(seen)
    s2[37] = seen[12]
    assert 12 not in TC.model6(pk[:41], s2[:41], [(p, t) for p, t in ops if p <= 41])["pending"]
    assert 12 not in r["pending"]  # and it ages out in the end


def test_segments_cover_the_stream():
    pk, seen, ops = TC.stream4()
    n = len(pk)
    for cut in range(n + 1):
        seg = TC.segments(n, ops, cut)
        assert [s[0] for s in seg] == [0] + [s[1] for s in seg[:-1]] and seg[-1][1] == n
        assert [t for s in seg for t in s[2]] == [t for _, t in ops]
        assert cut in (0, n) or any(s[1] == cut for s in seg)


def header_functions(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.findall(r"^int (gpk_\w+)\(", f.read(), re.M)


def test_new_symbols_declared_exported_and_listed():
    assert NEW[0] in header_functions("gpk_defrag.h") and NEW[1] in header_functions("gpk_defrag6.h")
    assert NEW[2] in header_functions("gpk_tcpasm.h")
    L = _lib.lib()
    for n in NEW:
        assert n in _lib.EXPORTS and hasattr(L, n), n
        assert getattr(L, n).argtypes is not None
    assert L.gpk_abi_version() == 2


@pytest.mark.parametrize("header,struct,cls", [("gpk_defrag.h", "gpk_defrag_time", _lib.DefragTime),
                                               ("gpk_defrag6.h", "gpk_defrag6_time", _lib.DefragTime),
                                               ("gpk_tcpasm.h", "gpk_tcpasm_time", _lib.TcpasmTime)])
def test_time_struct_matches_python(tmp_path, header, struct, cls):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    fields = [n for n, _ in cls._fields_]
    lines = ["#include <stddef.h>", "#include <stdio.h>", "#include <time.h>", '#include "%s"' % header,
             "int main(void) {", '  printf("{\\"size\\": %%zu", sizeof(%s));' % struct]
    lines += ['  printf(", \\"%s\\": %%zu", offsetof(%s, %s));' % (f, struct, f) for f in fields]
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout)
    assert got.pop("size") == ctypes.sizeof(cls)
    for f in fields:
        assert got[f] == getattr(cls, f).offset, f


def test_timed_calls_check_their_arguments():
    """No device needed: the argument checks come first."""
    L = _lib.lib()
    assert L.gpk_defrag_batch_timed(None, None, None, None, None, None, None) == _lib.GPK_EINVAL
    assert L.gpk_defrag6_batch_timed(None, None, None, None, 0, None, None, None) == _lib.GPK_EINVAL
    assert L.gpk_tcpasm_batch_timed(None, None, None, None, None, None, None, None) == _lib.GPK_EINVAL


# ---- TCP


def test_flush_with_options_comment_example():
    """assembly.go:216-226 as real frames: processed through 10, pages [15,20)
    [20,25) [30,50). The old first page pushes [15,25) with Skip 5; [30,50) stays
    while it is young, and goes with Skip 5 once it is old too."""
    pk, seen, names = TT.boundary_keys()
    r = TT.model(pk, seen, [(len(pk), TT.ts(TT.EDGE), True)])
    st = r["streams"][names["comment"]]
    assert [(c["len"], c["skip"], c["call"]) for c in st["chunks"]] == [
        (5, 0, st["first"]), (5, 5, ("flush", 0, 0)), (5, 0, ("flush", 0, 0))]
    assert st["data"] == b"hellofffffggggg" and st["closed"] == MT.OPEN
    g = st["group"]
    assert r["conn_seq"][g] == 25 and [p for p in r["pend"] if p[0] == st["first"] + 3] == [(st["first"] + 3, 0)]
    st = r["streams"][names["comment-old"]]
    assert [(c["len"], c["skip"], c["call"]) for c in st["chunks"]] == [
        (5, 0, st["first"]), (5, 5, ("flush", 0, 0)), (5, 0, ("flush", 0, 0)), (20, 5, ("flush", 0, 1))]
    assert st["closed"] == MT.OPEN and r["conn_seq"][st["group"]] == 50  # its lastSeen is young


def test_boundary_keys_by_hand():
    pk, seen, names = TT.boundary_keys()
    T = TT.ts(TT.EDGE)
    want2 = {"first==T": "untouched", "first==T-1": "closed by CloseAll", "drained==T": "untouched",
             "drained==T-1": "closed by CloseAll", "nosyn": "flushed", "multipage": "closed by CloseAll",
             "shield": "shielded", "fin": "closed by End", "comment": "flushed", "comment-old": "flushed",
             "young": "untouched"}
    r2 = TT.model(pk, seen, [(len(pk), T, True)])
    assert {n: r2["events"][0][j] for n, j in names.items()} == want2
    assert r2["flushes"] == [(7, 4)]
    r1 = TT.model(pk, seen, [(len(pk), T, False)])  # mode 1: the drained ones stay
    want1 = dict(want2, **{"first==T-1": "flushed", "drained==T-1": "untouched", "multipage": "flushed"})
    assert {n: r1["events"][0][j] for n, j in names.items()} == want1
    assert r1["flushes"] == [(6, 1)]
    ch = {n: r2["streams"][j]["chunks"] for n, j in names.items()}
    assert [c["skip"] for c in ch["first==T-1"]] == [0, 4] and [c["skip"] for c in ch["nosyn"]] == [-1]
    assert [(c["src_off"], c["len"], c["skip"]) for c in ch["multipage"][1:]] == [(0, 1900, 100), (1900, 1900, 0),
                                                                                   (3800, 1200, 0)]
    assert len({c["seen"] for c in ch["multipage"][1:]}) == 1 and all(c["call"] == ("flush", 0, 0) for c in ch["multipage"][1:])
    assert r2["streams"][names["first==T-1"]]["closed"] == ("flush", 0, 1)
    assert r2["streams"][names["fin"]]["closed"] == ("flush", 0, 0) and ch["fin"][-1]["flags"] & MT.END
    g = r2["streams"][names["drained==T"]]["group"]
    assert r2["conn_last_seen"][g] == T
    # the same with a page limit: time and MaxBufferedPagesPerConnection together
    r3 = TT.model(pk, seen, [(len(pk), T, True)], max_pages=2)
    assert r3["flushes"][0][0] >= 5 and r3["streams"][names["multipage"]]["chunks"] != ch["multipage"]


def test_last_seen_is_a_maximum():
    pk, seen, want = TT.last_seen_keys()
    r = TT.model(pk, seen)
    assert r["conn_last_seen"] == want and r["counts"][4] == len(want) and r["counts"][3] == 0
    assert len(pk) == 131 * len(want)


def test_long_list_rounds():
    pk, seen, T = TT.long_list()
    r = TT.model(pk, seen, [(len(pk), T, True)])
    st = r["streams"][0]
    assert r["flushes"] == [(1, 0)] and len(st["chunks"]) == 270 and len(r["pend"]) == 30
    assert [c["call"] for c in st["chunks"]] == [("flush", 0, j) for j in range(270)]
    assert r["events"][0][0] == "flushed"


def test_stream_meets_every_condition():
    pk, seen, ops = TT.stream()
    r = TT.model(pk, seen, ops)
    kinds = {v for ev in r["events"] for v in ev.values()}
    assert kinds == {"untouched", "shielded", "flushed", "closed by End", "closed by CloseAll"}
    assert all(f > 0 for f, _ in r["flushes"]) and r["flushes"][1][1] <= r["flushes"][1][0]
    assert "closed by CloseAll" not in r["events"][1].values()  # the second flush has no CloseAll
    assert MT.QUEUED in r["verdict"] and MT.DIRECT in r["verdict"]
    for cut in (0, 50, 77, 150):
        seg = TT.segments(len(pk), ops, cut)
        assert seg[0][0] == 0 and seg[-1][1] == 150 and [k for s in seg for k in s[2]] == [0, 1, 2]


def test_free_list_rule():
    """recycle on and off agree on traffic whose timestamps never run backwards;
    the one hand-made backwards case shows where they part."""
    pk = tcpasmcases.random_traffic(7, 400)
    seen = [TT.ts(i) for i in range(len(pk))]
    n = len(pk)
    ops = [(n // 3, TT.ts(n // 3 - 40), True), (2 * n // 3, TT.ts(2 * n // 3 - 40), False), (n, TT.ts(n - 40), True)]
    a, b = TT.model(pk, seen, ops, recycle=False), TT.model(pk, seen, ops, recycle=True)
    assert sum(c for _, c in a["flushes"]) > 5 and a["counts"][0] > 400
    for k in ("verdict", "stream_of", "streams", "conn_seq", "conn_stream", "conn_last_seen", "pend", "flushes",
              "events", "log"):
        assert a[k] == b[k], k
    pk, seen = TT.backwards_case()
    ops = [(4, TT.ts(50), True)]
    dev, ref = TT.model(pk, seen, ops, recycle=False), TT.model(pk, seen, ops, recycle=True)
    # the device's rule: Y's lastSeen is its own 21 ms, Before(50 ms): closed. The reference's: Y inherited X's
    # 100 ms through the struct, not Before(50 ms): left open.
    assert dev["flushes"] == [(1, 1)] and dev["events"][0] == {1: "closed by CloseAll"} and dev["counts"][4] == 0
    assert ref["flushes"] == [(0, 0)] and ref["events"][0] == {1: "untouched"} and ref["counts"][4] == 1
    assert ref["conn_last_seen"] == [TTM.ZERO, TT.ts(100)] and dev["conn_last_seen"] == [TTM.ZERO, TTM.ZERO]
    assert dev["verdict"] == ref["verdict"] and dev["stream_of"] == ref["stream_of"]
