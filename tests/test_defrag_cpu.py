"""The reassembly model (tests/defrag_model.py) pinned on ip4defrag's own
tests (defrag_test.go:38-279): the expected out != nil pattern, the 4508-byte
payload, the Id, the struct tests' error / no-error outcomes, and the two
quirks checked against the reference's code by hand. Plus the C side of
include/gpk_defrag.h: it compiles as C11 and C++, and its struct and constants
match gopacket_amd/_lib.py. CPU only; the device path is tests/test_defrag_gpu.py."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import defrag_model as M
import defragcases as DC
import flowcases
import pktutil
from configs import oracle_parser
from gopacket_amd import _lib
from oracle import flows_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P1 = ["testPing1Frag1", "testPing1Frag3", "testPing1Frag2", "testPing1Frag4"]
# (name, frames in injection order, expect out != nil) — defrag_test.go:38-151, 264-279
SEQUENCES = {
    "TestDefragPing1": (P1 + P1, [False, False, False, True] * 2),
    "TestDefragPingMultipleFrags": (["testPing1Frag1"] * 3 + ["testPing1Frag3", "testPing1Frag2", "testPing1Frag4"],
                                    [False] * 5 + [True]),
    "TestDefragPing1and2": (["testPing1Frag1", "testPing1Frag3", "testPing2Frag3", "testPing2Frag4", "testPing1Frag2",
                             "testPing2Frag1", "testPing1Frag4", "testPing2Frag2"], [False] * 6 + [True, True]),
    "TestDefragIDField": (P1, [False, False, False, True]),
}


def run_model(packets, cfg=flowcases.DEFRAG_PARSER):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(cfg).decode(data, off, cap, layouts=True)
    return M.run(packets, res["records"], res["layouts"])


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_reference_sequences(name):
    frames, _ = flowcases.defrag_frames()
    order, expect = SEQUENCES[name]
    r = run_model([frames[k] for k in order])
    assert [v >= 0 for v in r["verdict"]] == expect
    assert all(v == M.HELD for v, e in zip(r["verdict"], expect) if not e)
    assert len(r["datagrams"]) == sum(expect) and not r["pending"]
    for d in r["datagrams"]:
        which = DC.PING1 if order[d["last"]] in DC.PING1 else DC.PING2
        assert len(d["payload"]) == 4508 and d["length"] == 4508
        assert d["payload"] == b"".join(frames[k][34:] for k in which)
        # out takes its fields from `in`: Id (TestDefragIDField), and the header is in's
        assert d["data"][18:20] == frames[which[0]][18:20]
        assert d["payload_off"] == 34 and d["data"][34:] == d["payload"]
        assert d["data"][20:22] == b"\x00\x00" and flowcases.csum(d["data"][14:34]) == 0
        assert int.from_bytes(d["data"][16:18], "big") == 20 + 4508


def test_struct_tests_error_outcomes():
    cases = dict(flowcases.defrag_struct_cases())

    def verdicts(*labels):
        return run_model([cases[l] for l in labels])["verdict"]

    assert verdicts("TestNotFrag (DF)") == [FO.NONE]                                  # out == in, no error
    assert verdicts("TestDefragTooSmall Length 27 MF", "TestDefragTooSmall Length 28 MF") == [FO.FRAG_TOO_SMALL, M.HELD]
    assert verdicts("TestDefragSmallFinalFragment") == [FO.NONE]                      # no error
    assert verdicts("TestDefragFragmentOffset 0", "TestDefragFragmentOffset 8184") == [M.HELD, FO.FRAG_OFFSET]
    assert verdicts("TestDefragMaxSize Length 65535", "TestDefragMaxSize Length 28 off 1") == [M.HELD, M.HELD]


def test_counted_but_not_listed():
    """MF offset 0 with 64 bytes, then MF offset 4 (32 < Highest 64, no larger
    entry): the second is not listed, yet Current becomes 80."""
    pk = [DC.frag(7, 0, 1, b"a" * 64), DC.frag(7, 4, 1, b"b" * 16)]
    r = run_model(pk)
    assert r["verdict"] == [M.HELD, M.HELD]
    (lst,), (state,) = r["lists"].values(), r["state"].values()
    assert lst == [0] and state == (64, 80, False)
    assert r["pending"] == [0, 1]


def test_maximum_list_length_is_reachable():
    """8192 copies of an MF fragment at FragOffset 8183 with Length 100:
    Highest wraps to 8, every copy is pushed, the 8192nd flushes the key."""
    pk = [DC.frag(9, 8183, 1, b"c" * 80)] * M.MAX_LIST + [DC.frag(9, 8183, 1, b"c" * 80)]
    r = run_model(pk)
    assert r["verdict"][:M.MAX_LIST - 1] == [M.HELD] * (M.MAX_LIST - 1)
    assert r["verdict"][M.MAX_LIST - 1] == M.EMAXLEN
    assert r["verdict"][M.MAX_LIST] == M.HELD and r["pending"] == [M.MAX_LIST]


@pytest.mark.parametrize("name", sorted(DC.quirk_cases()))
def test_build_branches(name):
    pk, verdict, pending = DC.quirk_cases()[name]
    r = run_model(pk)
    assert r["verdict"] == verdict and r["pending"] == pending
    assert len(r["datagrams"]) == sum(v >= 0 for v in verdict)
    if name == "overlap that completes":
        assert r["datagrams"][0]["payload"] == b"x" * 24 + b"z" * 8 and r["datagrams"][0]["length"] == 48
    if name == "duplicates":
        assert r["datagrams"][0]["payload"] == b"p" * 16 + b"r" * 5


def test_header_compiles_as_c11_and_cxx(tmp_path):
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if not shutil.which(cc):
            pytest.skip("needs " + cc)
        src = tmp_path / ("hdr." + ext)
        src.write_text('#include "gpk_defrag.h"\nint main(void) { gpk_datagrams d; (void)d; return GPK_DEFRAG_HELD + 16; }\n')
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                            str(tmp_path / "hdr.o"), str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_struct_and_constants_match_python(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    fields = [n for n, _ in _lib.Datagrams._fields_]
    consts = dict(GPK_DEFRAG_HELD=_lib.DEFRAG_HELD, GPK_DEFRAG_EHOLE=_lib.DEFRAG_EHOLE,
                  GPK_DEFRAG_EINVALID=_lib.DEFRAG_EINVALID, GPK_DEFRAG_EMAXLEN=_lib.DEFRAG_EMAXLEN,
                  GPK_DEFRAG_EPANIC=_lib.DEFRAG_EPANIC, GPK_DEFRAG_MAX_LIST=_lib.DEFRAG_MAX_LIST)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gpk_defrag.h"', "int main(void) {",
             '  printf("{\\"size\\": %zu", sizeof(gpk_datagrams));']
    lines += ['  printf(", \\"%s\\": %%zu", offsetof(gpk_datagrams, %s));' % (f, f) for f in fields]
    lines += ['  printf(", \\"%s\\": %%d", (int)%s);' % (c, c) for c in consts]
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout)
    assert got.pop("size") == ctypes.sizeof(_lib.Datagrams)
    for f in fields:
        assert got[f] == getattr(_lib.Datagrams, f).offset, f
    for c, v in consts.items():
        assert got[c] == v, c
    assert M.HELD == _lib.DEFRAG_HELD and M.EPANIC == _lib.DEFRAG_EPANIC and M.MAX_LIST == _lib.DEFRAG_MAX_LIST
