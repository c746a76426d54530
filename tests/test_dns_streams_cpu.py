"""DNS over reassembled streams without a GPU: gpk_dns_streams_host (the C++ the
kernels run, on the calling thread) against the model (dnsstream_model.py) on
every case of dnsstreamcases.py, on the reference's own message vectors and on
a seeded mix, byte for byte; the terminal rules by hand; both capacity levels
and the retry; max_msg_len; the TOOBIG and bad-tail paths, argument faults, the
ABI layout, the exports, and the per-packet pass, which the templated rules
must leave as it was."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dns_model as M
import dnscases as C
import dnsstream_model as SM
import dnsstreamcases as SC
from dnsstreamutil import ARENAS, HostChain, assert_same_streams, mix_case, run_case_host
from dnsutil import GOLDEN, assert_same_dns, golden_packet, model_and_host
from gopacket_amd import _lib, flows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in SC.cases()}
D = flows.DNSStreamDecoder
NQ, NR = 1, 7  # entries of query() and of response()


@pytest.mark.parametrize("name", list(CASES))
def test_host_matches_model(name):
    run_case_host(CASES[name])


def states(res):
    return [d["state"] for d in res]


def kinds(d):
    """Per entry: "ok", the error code, or the PARTIAL / SKIPPED status as a negative number."""
    return ["ok" if "msg" in e else e["err"] if "err" in e else -e["mstatus"] for e in d["entries"]]


@pytest.mark.parametrize("two", [False, True], ids=["one_call", "two_calls"])
def test_every_split_position_gives_the_same_messages(two):
    """One stream per cut position of a query and a six-entry response: each
    yields the same two messages, whether the two segments come in one call or
    in two. The per-packet pass decodes the length bytes of the query's packet
    as the ID and fails."""
    calls = run_case_host(CASES["split_two_calls" if two else "split_one_call"])
    n = len(SC.exchange()) - 1
    got = {}
    for res in calls:
        assert len(res) == n and set(states(res)) == {SM.SYNCED}
        for d in res:
            got.setdefault(d["id"], []).extend((e["len"], e["msg"]["id"], len(e["msg"]["rrs"])) for e in d["entries"])
    want = [(29, 0x1234, NQ), (len(SC.response()), 0x1234, NR)]
    assert all(got[g] == want for g in range(n)), [g for g in range(n) if got[g] != want][:5]
    if two:  # half a prefix, a prefix and no body, then every later position
        Q = 2 + 29
        assert [len(d["tail"]) for d in calls[0]] == [k if k < Q else k - Q for k in range(1, n + 1)]
        assert all(d["tail_in"] == len(t["tail"]) for d, t in zip(calls[1], calls[0]))
    m, h, _ = model_and_host(C.PARSER, [C.over_tcp(SC.query())])
    assert_same_dns(m, h)
    # the length bytes read as the ID shift everything by two: 0x0100 questions, and the decode fails
    assert int(m["counts"][0]) == 1 and int(m["records"][0]["err"]) != 0


def test_the_response_has_the_six_record_types():
    (res,) = run_case_host(CASES["exchange"])
    rrs = res[0]["entries"][1]["msg"]["rrs"]
    assert [r["type"] for r in rrs] == [C.A, C.A, C.AAAA, C.CNAME, C.MX, C.TXT, C.OPT]
    assert rrs[3]["rname"] == b"www.example.com" and rrs[4]["rname"] == b"mail.example.com" and rrs[4]["v"][0] == 10
    assert rrs[5]["count"] == 2 and rrs[6]["count"] == 1
    assert SM.questions(res) == [(0, b"example.com", C.A)] * 2


def test_pointers_across_the_seam():
    a, b = run_case_host(CASES["seam_pointers"])
    assert [len(d["tail"]) for d in a] == [31, 18] and [d["tail_in"] for d in b] == [31, 18]
    for d in b:  # the pointers at offset 12 resolve through the carried tail
        (e,) = d["entries"]
        assert [r["name"] for r in e["msg"]["rrs"]] == [b"example.com"] * 6 + [b""]
        assert e["msg"]["rrs"][3]["rname"] == b"www.example.com"


def test_tail_is_bounded_by_the_16_bit_length():
    calls = run_case_host(CASES["largest_message"])
    assert [len(res[0]["tail"]) for res in calls] == [20 * SC.MSS, 65536, 0]
    assert _lib.DNSS_MAX_TAIL == SM.MAX_TAIL == 2 + 65535 - 1 == 65536
    big, small = calls[2][0]["entries"]
    assert (big["len"], big["msg"]["rrs"][1]["data_length"], small["len"]) == (65535, 65535 - 41, 29)
    assert big["msg"]["rrs"][1]["count"] == 256
    hdr = open(os.path.join(ROOT, "include", "gpk_dns_streams.h")).read()
    assert re.search(r"#define GPK_DNSS_MAX_TAIL 65536u", hdr)


def test_terminal_rules_by_hand():
    r = {n: run_case_host(CASES[n]) for n in (
        "length_0_and_11", "max_message", "loss_in_front", "loss_inside", "loss_behind", "page_limit_forces_a_skip",
        "close_whole", "close_partial", "loss_and_close", "no_syn", "no_syn_framed", "server_direction", "port_table",
        "port_8080_and_80")}
    (a,) = r["length_0_and_11"]  # both short messages fail on their own and framing goes on
    assert kinds(a[0]) == [M.E_SHORT, M.E_SHORT, "ok"] and [e["len"] for e in a[0]["entries"]] == [0, 11, 29]
    assert [e["hdr_off"] for e in a[0]["entries"]] == [2, 4, 17]
    (a,) = r["max_message"]  # at the limit it decodes, one byte over it is framed over
    assert kinds(a[0]) == ["ok", -SM.SKIPPED, "ok"] and a[0]["entries"][1]["len"] == len(SC.response()) + 1
    a, b = r["loss_in_front"]
    assert states(b) == [SM.LOST] and b[0]["entries"] == []
    a, b = r["loss_inside"]  # the bytes in front of the gap: a prefix and 8 bytes of the query
    assert states(a) == [SM.SYNCED] and states(b) == [SM.LOST] and kinds(b[0]) == [-SM.PARTIAL]
    assert (b[0]["entries"][0]["len"], b[0]["entries"][0]["present"]) == (29, 10)
    a, b = r["loss_behind"]
    assert kinds(a[0]) == ["ok", "ok"] and states(b) == [SM.LOST] and b[0]["entries"] == []
    a, b = r["page_limit_forces_a_skip"]  # the messages in front of the gap, one partial entry, then nothing
    assert states(a) == [SM.LOST] and kinds(a[0])[:2] == ["ok", "ok"] and kinds(a[0])[-1] == -SM.PARTIAL
    assert states(b) == [SM.LOST] and b[0]["entries"] == [] and not b[0]["framed"]
    (a,) = r["close_whole"]
    assert states(a) == [SM.CLOSED] and kinds(a[0]) == ["ok", "ok"]
    (a,) = r["close_partial"]
    assert states(a) == [SM.CLOSED] * 3 and all(kinds(d) == ["ok", "ok", -SM.PARTIAL] for d in a)
    assert [(d["entries"][2]["len"], d["entries"][2]["present"]) for d in a] == [(len(SC.response()), 60), (0, 1), (29, 2)]
    a, b = r["loss_and_close"]  # a loss wins over a close
    assert states(b) == [SM.LOST] and kinds(b[0]) == [-SM.PARTIAL]
    assert states(r["no_syn"][1]) == [SM.NOSTART] and r["no_syn"][1][0]["entries"] == []
    assert states(r["no_syn_framed"][1]) == [SM.CLOSED] and kinds(r["no_syn_framed"][1][0]) == ["ok", "ok"]
    (a,) = r["server_direction"]
    assert states(a) == [SM.SYNCED] and kinds(a[0]) == ["ok", "ok"]
    (a,) = r["port_table"]  # 5353 registered, 53 unregistered
    assert states(a) == [SM.SYNCED, SM.NONE] and kinds(a[0]) == ["ok", "ok"] and not a[1]["framed"]
    (a,) = r["port_8080_and_80"]
    assert states(a) == [SM.SYNCED, SM.NONE]


def test_quirk_streams_cover_the_errors():
    """The hand-built messages of dnscases fail over a stream with the error
    they fail with in a datagram, and the reference's text."""
    (res,) = run_case_host(CASES["quirks"])
    seen = {e["err"] for d in res for e in d["entries"] if "err" in e}
    short = {M.E_MAXREC}  # needs a chain longer than the cases here carry (QUIRK_MAX)
    assert seen >= set(M.ALL_ERRORS) - short, set(M.ALL_ERRORS) - seen
    buf = ctypes.create_string_buffer(256)
    for d in res:
        for e in d["entries"]:
            if "err" in e:
                n = _lib.lib().gpk_dns_format_error(e["err"], e["err_a0"], e["err_a1"], buf, 256)
                assert n == len(buf.value) and buf.value.decode() == M.error_text(e["err"], e["err_a0"], e["err_a1"])
    assert set(states(res)) == {SM.CLOSED}


def test_reference_vectors_over_streams():
    """The reference's own message vectors (tests/golden/dns_vectors.json), each
    behind a length prefix in a stream of its own, cut inside the message."""
    msgs = []
    for v in GOLDEN:
        pkt, at = golden_packet(v)
        msgs.append(pkt[at:])
    assert len(msgs) > 10
    pk = [f for i, m in enumerate(msgs) for f in SC.conn(i, SC.pre(m), [7], dport=53, fin=True)]
    (res,) = run_case_host(mix_case([pk], flush=False))
    assert len(res) == len(msgs) and set(states(res)) == {SM.CLOSED}
    ok = 0
    for d, m in zip(res, msgs):
        (e,) = d["entries"]
        assert e["len"] == len(m)
        try:
            want = M.decode_message(m, 2)
            assert e["msg"] == want
            ok += 1
        except M.GoError as x:
            assert e["err"] == x.code
    assert ok > len(msgs) // 2


@pytest.fixture(scope="module")
def mix():
    return SC.random_mix(20261021, 300)


def test_random_mix_in_three_calls(mix):
    calls = run_case_host(mix_case(mix))
    every = [d for res in calls for d in res]
    ents = [e for d in every for e in d["entries"]]
    # from the model alone: the mix is only meaningful if most of it decodes, and if every state occurs
    assert 3 * sum("msg" in e for e in ents) >= len(ents) > 500
    assert {d["state"] for d in every} == {SM.SYNCED, SM.NONE, SM.NOSTART, SM.LOST, SM.CLOSED}
    assert sum(len(d["tail"]) > 0 for d in every) > 50 and sum(d["tail_in"] > 0 and d["entries"] != [] for d in every) > 30
    assert {-SM.PARTIAL, "ok", M.E_SHORT} <= {k for d in every for k in kinds(d)}


def one_call(pk, **kw):
    model = SM.Streaming(SC.PARSER, 0, **kw)
    model.feed(pk)
    return model.last


def cap_packets(n):
    return [f for i in range(n) for f in SC.conn(i, SC.exchange(i) + SC.pre(SC.query())[:3 + i % 5], [40 + i], dport=53)]


def test_capacity_rules_both_levels():
    """Each arena in turn at exact, at exact - 1 and at 0. Level one: a stream's
    message entries and tail are written whole or not at all. Level two: a
    placed message's entries and names are written whole or not at all.
    Nothing is written at or past a capacity, counts names the need of what
    was placed, and the retry helper gets everything."""
    last = one_call(cap_packets(6))
    full, hfull = HostChain(SC.PARSER).call(last, keep=False)
    need = D.needed(hfull["counts"])
    assert need == tuple(len(full[k]) for k in ARENAS) and need[0] == 12 and need[1] == 6 * (NQ + NR) and min(need) > 0
    assert not int(hfull["counts"][4]) and not np.any(hfull["streams"][:6]["status"]) and not np.any(hfull["msgs"]["status"])
    for k in range(4):
        for caps in (need, tuple(x - (j == k) for j, x in enumerate(need)), tuple(0 if j == k else x for j, x in enumerate(need))):
            m, h = HostChain(SC.PARSER).call(last, caps=caps, keep=False)
            assert_same_streams(m, h, "caps %r" % (caps,))
            short = caps != need
            assert int(h["counts"][4]) == int(short)
            st = h["streams"][:6]
            sdrop = (st["status"] & _lib.DNSS_ST_DROPPED) != 0
            placed = int(sum(int(t["nmsg"]) for t in st[~sdrop]))
            mdrop = (h["msgs"][:placed]["status"] & _lib.DNSS_MSG_DROPPED) != 0
            assert bool(sdrop.any()) == (short and k in (0, 3)) and bool(mdrop.any()) == (short and k in (1, 2))
            got = D.needed(h["counts"])
            assert (got[0], got[3]) == (need[0], need[3])  # the stream level's needs are always whole
            if not sdrop.any():
                assert got == need
            if short and caps[k] == need[k] - 1:  # only the last stream, or the last message, does not fit
                assert list(sdrop) == ([False] * 5 + [True] if k in (0, 3) else [False] * 6)
                assert list(mdrop) == ([False] * 11 + [True] if k in (1, 2) else [False] * placed)
            for t in st[~sdrop]:  # what was kept is what the full run wrote
                a, b = int(t["msg0"]), int(t["msg0"]) + int(t["nmsg"])
                assert b <= caps[0]
                a, b = int(t["tail_off"]), int(t["tail_off"]) + int(t["tail_len"])
                assert b <= caps[3] and h["tails"][a:b].tobytes() == hfull["tails"][a:b].tobytes()
            for e, f in zip(h["msgs"][:placed][~mdrop], hfull["msgs"][:placed][~mdrop]):
                assert e.tobytes() == f.tobytes()
                a, b = int(e["msg"]["rr0"]), int(e["msg"]["rr0"]) + int(e["msg"]["nrr"])
                assert b <= caps[1] and h["rrs"][a:b].tobytes() == hfull["rrs"][a:b].tobytes()
            assert list(st["state"]) == list(hfull["streams"][:6]["state"])  # state and sizes are set all the same
            assert list(st["nmsg"]) == list(hfull["streams"][:6]["nmsg"])
    data, off, cap, ref = last["arrays"]
    asm = SM.asm_arrays(last["asm"], len(cap))
    p = HostChain(SC.PARSER).parser
    out = D.decode_host_all(p, data, off, cap, ref["records"], ref["layouts"], asm)
    assert not int(out["counts"][4])
    for k in ARENAS:
        assert out[k].tobytes() == hfull[k].tobytes(), k
    # the first call of the retry sizes the streams, the second the messages
    a = D.decode_host(p, data, off, cap, ref["records"], ref["layouts"], asm, 0, 0, 0, 0)
    assert D.needed(a["counts"]) == (need[0], 0, 0, need[3]) and int(a["counts"][4]) == 1 and int(a["counts"][3]) == 0
    b = D.decode_host(p, data, off, cap, ref["records"], ref["layouts"], asm, need[0], 0, 0, need[3])
    assert D.needed(b["counts"]) == need and int(b["counts"][4]) == 1


def test_max_msg_len_by_hand():
    pk = SC.conn(1, SC.pre(SC.response()) + SC.pre(SC.query()), [50], dport=53)
    for lim, want in ((0, ["ok", "ok"]), (len(SC.response()), ["ok", "ok"]), (len(SC.response()) - 1, [-SM.SKIPPED, "ok"]),
                      (28, [-SM.SKIPPED, -SM.SKIPPED]), (65535, ["ok", "ok"])):
        case = mix_case([pk], flush=False, max_message=lim)
        (res,) = run_case_host(case)
        assert kinds(res[0]) == want, lim
    last = one_call(pk)
    data, off, cap, ref = last["arrays"]
    with pytest.raises(_lib.GpkError):  # a limit that a 16-bit length cannot reach
        D.decode_host(HostChain(SC.PARSER).parser, data, off, cap, ref["records"], ref["layouts"],
                      SM.asm_arrays(last["asm"], len(cap)), 8, 8, 64, 64, max_message=65536)


def test_toobig_is_lost_without_reading_a_byte():
    """A forged stream_data0 with no bytes behind it: a logical buffer of 2^32
    bytes or more is TOOBIG and treated as LOST; so is a stream past data_cap,
    and a tail that does not lie in the arena."""
    last = one_call(SC.conn(1, SC.exchange(), [50], dport=53) + SC.conn(2, SC.exchange(), [60], dport=53))
    data, off, cap, ref = last["arrays"]
    p = HostChain(SC.PARSER).parser
    asm = SM.asm_arrays(last["asm"], len(cap))
    end = int(asm["stream_data0"][2])
    for forged, cap_, want in (([0, 0, 1 << 32], 1 << 33, [SM.SYNCED, SM.LOST]),
                               ([0, 1 << 32, 1 << 32], 1 << 33, [SM.LOST, SM.SYNCED]),
                               ([0, end // 2, end], end - 1, [SM.SYNCED, SM.LOST])):
        a = dict(asm, stream_data0=np.array(forged + [0] * (len(cap) - 2), np.uint64), data_cap=cap_,
                 data=np.zeros(0, np.uint8) if cap_ > end else asm["data"], chunks=asm["chunks"][:0], chunk_cap=0,
                 counts=np.array([2, 0, 0, 0, 0, 0, 0, 0], np.uint64))
        h = D.decode_host(p, data, off, cap, ref["records"], ref["layouts"], a, 8, 64, 256, 64)
        st = h["streams"][:2]
        assert list(st["state"]) == want, forged
        big = st[st["state"] == SM.LOST][0]
        assert int(big["status"]) == _lib.DNSS_ST_TOOBIG and int(big["nmsg"]) == 0 and int(big["tail_len"]) == 0
        assert int(h["counts"][0]) == 2 and int(h["counts"][1]) == 2
    carry = (np.array([SM.SYNCED, SM.SYNCED], np.uint32), np.array([0, 6], np.uint64), np.array([4, 5], np.uint32),
             np.zeros(10, np.uint8))
    h = D.decode_host(p, data, off, cap, ref["records"], ref["layouts"], dict(asm), 8, 64, 256, 64, carry=carry)
    assert [int(x) for x in h["streams"][:2]["status"]] == [0, _lib.DNSS_ST_BADTAIL]
    assert [int(x) for x in h["streams"][:2]["state"]] == [SM.SYNCED, SM.LOST]
    # four zero bytes in front: two empty messages, then the stream's own
    assert [int(x) for x in h["msgs"][:4]["msg"]["err"]] == [M.E_SHORT, M.E_SHORT, 0, 0]


def test_host_argument_checks():
    last = one_call(SC.conn(1, SC.exchange(), [50], dport=53))
    data, off, cap, ref = last["arrays"]
    n = len(cap)
    p = HostChain(SC.PARSER).parser
    asm = SM.asm_arrays(last["asm"], n)
    good = D.decode_host(p, data, off, cap, ref["records"], ref["layouts"], asm, 8, 16, 256, 64)
    assert D.needed(good["counts"])[:2] == (2, NQ + NR) and list(good["counts"][:5]) == [1, 1, 2, 0, 0]
    lib = _lib.lib()
    b = _lib.Batch(data.ctypes.data, off.ctypes.data, cap.ctypes.data, n, data.size)
    r = _lib.Results(ref["records"].ctypes.data, None, None, ref["layouts"].ctypes.data)
    keys = D.ASM_KEYS

    def call(parser=p, batch=b, inp=None, asm_kw=(), **kw):
        av = {k: asm[k].ctypes.data if k in asm else None for k in keys}
        av.update(asm_kw)
        a = _lib.TcpStreams(*[av[k] for k in keys], asm["chunk_cap"], asm["data_cap"])
        o = dict(streams=good["streams"].ctypes.data, msgs=good["msgs"].ctypes.data, rrs=good["rrs"].ctypes.data,
                 names=good["names"].ctypes.data, tails=good["tails"].ctypes.data, counts=good["counts"].ctypes.data,
                 msg_cap=8, rr_cap=16, name_cap=256, tail_cap=64)
        o.update(kw)
        return lib.gpk_dns_streams_host(parser.h if parser else None, ctypes.byref(batch), ctypes.byref(r), ctypes.byref(a),
                                        ctypes.byref(inp) if inp is not None else None, ctypes.byref(_lib.DnsStreamOut(**o)))
    assert call() == 0
    odd = good["msgs"].ctypes.data + 4
    for kw in (dict(streams=None), dict(counts=None), dict(msgs=None), dict(rrs=None), dict(names=None),
               dict(tails=None), dict(msgs=odd), dict(rrs=odd), dict(streams=good["streams"].ctypes.data + 4),
               dict(msg_cap=1 << 28),
               dict(asm_kw=dict(counts=None)), dict(asm_kw=dict(chunks=None)), dict(asm_kw=dict(stream_first=None)),
               dict(asm_kw=dict(stream_closed=None)), dict(asm_kw=dict(stream_data0=None)), dict(asm_kw=dict(data=None)),
               dict(parser=None)):
        assert call(**kw) == _lib.GPK_EINVAL, kw
    assert call(msgs=None, msg_cap=0) == 0 and call(rrs=None, rr_cap=0) == 0 and call(names=None, name_cap=0) == 0
    assert call(tails=None, tail_cap=0) == 0
    st = np.zeros(n + 1, np.uint32)
    z8, z4 = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    mk = lambda **kw: _lib.DnsStreamIn(**dict(dict(state=st.ctypes.data, tail_off=z8.ctypes.data,  # noqa: E731
                                                    tail_len=z4.ctypes.data, tails=None, n=1, tail_bytes=0, flags=0,
                                                    max_msg_len=0), **kw))
    assert call(inp=mk()) == 0 and call(inp=mk(flags=_lib.DNSS_FRAME_UNSTARTED)) == 0 and call(inp=mk(max_msg_len=65535)) == 0
    for bad in (mk(flags=2), mk(n=n + 1), mk(state=None), mk(tail_off=None), mk(tail_len=None), mk(tail_bytes=4),
                mk(max_msg_len=65536)):
        assert call(inp=bad) == _lib.GPK_EINVAL
    empty = _lib.Batch(None, None, None, 0, 0)
    assert call(batch=empty) == 0 and list(good["counts"]) == [0] * 12


def test_abi_layout_of_dns_stream_structs(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler (gcc, cc or clang): the build needs a host compiler too"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_dns_streams.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_dns_stream", _lib.DNS_STREAM_DTYPE), ("gpk_dns_stream_msg", _lib.DNS_STREAM_MSG_DTYPE),
                          ("gpk_dns_stream_in", _lib.DnsStreamIn), ("gpk_dns_stream_out", _lib.DnsStreamOut)):
        if isinstance(mirror, np.dtype):
            size, fields = mirror.itemsize, {n: mirror.fields[n][1] for n in mirror.names}
        else:
            size, fields = ctypes.sizeof(mirror), {n: getattr(mirror, n).offset for n, *_ in mirror._fields_}
        want[cname] = [size] + list(fields.values())
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f in fields:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.splitlines()}
    assert got == want
    assert (_lib.DNS_STREAM_DTYPE.itemsize, _lib.DNS_STREAM_MSG_DTYPE.itemsize) == (64, 80)
    assert _lib.DNS_STREAM_MSG_DTYPE.fields["msg"][0] == _lib.DNS_DTYPE  # the first 64 bytes, unchanged
    assert _lib.DNS_STREAM_MSG_DTYPE.itemsize % 8 == 0


def test_exports_and_constants():
    for name in ("gpk_dns_stream_decoder_create", "gpk_dns_stream_decoder_destroy", "gpk_dns_streams",
                 "gpk_dns_streams_host"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "gpk_dns_streams.h")).read()
    for cname, val in (("GPK_DNSS_NEW", _lib.DNSS_NEW), ("GPK_DNSS_SYNCED", _lib.DNSS_SYNCED),
                       ("GPK_DNSS_NONE", _lib.DNSS_NONE), ("GPK_DNSS_NOSTART", _lib.DNSS_NOSTART),
                       ("GPK_DNSS_LOST", _lib.DNSS_LOST), ("GPK_DNSS_CLOSED", _lib.DNSS_CLOSED),
                       ("GPK_DNSS_NSTATE", _lib.DNSS_NSTATE),
                       ("GPK_DNSS_ST_DROPPED", _lib.DNSS_ST_DROPPED), ("GPK_DNSS_ST_TOOBIG", _lib.DNSS_ST_TOOBIG),
                       ("GPK_DNSS_ST_BADTAIL", _lib.DNSS_ST_BADTAIL), ("GPK_DNSS_MSG_PARTIAL", _lib.DNSS_MSG_PARTIAL),
                       ("GPK_DNSS_MSG_SKIPPED", _lib.DNSS_MSG_SKIPPED), ("GPK_DNSS_MSG_DROPPED", _lib.DNSS_MSG_DROPPED),
                       ("GPK_DNSS_FRAME_UNSTARTED", _lib.DNSS_FRAME_UNSTARTED), ("GPK_DNSS_MAX_TAIL", _lib.DNSS_MAX_TAIL)):
        assert re.search(r"#define %s %su?\s" % (cname, val), hdr), cname
    assert "NOT_DNS" not in hdr.replace("no \"not DNS\" state", "")
    assert (SM.NEW, SM.SYNCED, SM.NONE, SM.NOSTART, SM.LOST, SM.CLOSED) == tuple(range(6))
    assert (SM.PARTIAL, SM.SKIPPED, SM.DROPPED) == (_lib.DNSS_MSG_PARTIAL, _lib.DNSS_MSG_SKIPPED, _lib.DNSS_MSG_DROPPED)
    assert _lib.DNS_ERR_END - _lib.DNS_ERR_FIRST == 31  # no error code was added
    for cls in (flows.DNSStreamDecoder, flows.DNSStreams, flows.DNSStreamResult):
        assert cls.__doc__
    for name in ("decode", "decode_all", "decode_host", "decode_host_all", "needed"):
        assert callable(getattr(flows.DNSStreamDecoder, name))
    for name in ("feed", "flush_all", "flush_older_than", "close"):
        assert callable(getattr(flows.DNSStreams, name))
    for name in ("messages", "questions"):
        assert callable(getattr(flows.DNSStreamResult, name))
    # the carry logic is one class for both stream passes
    assert flows.DNSStreams.feed is flows.TLSStreams.feed and flows.DNSStreams._carry_in is flows.TLSStreams._carry_in


def test_per_packet_pass_is_unchanged():
    """The rules became templates on the byte source: gpk_dns_batch_host still
    equals its model on the hand-built cases and on the seeded corpus."""
    cases = [p for _, p in C.quirk_cases()[0]]
    m, h, _ = model_and_host(C.PARSER, cases, fill=0xA5)
    assert_same_dns(m, h, "cases")
    m, h, _ = model_and_host(C.PARSER, C.fuzz_packets(C.FUZZ_SEED, 1024), align=16, pad=3, fill=0xA5)
    assert_same_dns(m, h, "fuzz")
    assert int(m["counts"][1]) > 100 and int(m["counts"][2]) > 100
