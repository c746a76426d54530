"""TLS over reassembled streams without a GPU: gpk_tls_streams_host (the C++ the
kernels run, on the calling thread) against the model (tlsstream_model.py) on
every case of tlsstreamcases.py and on a seeded mix, byte for byte; the
terminal rules by hand; the capacity rules, the TOOBIG path, argument faults,
error texts, the ABI layout, and the per-packet pass, which the shared record
body must leave as it was."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tls_model as M
import tlscases as C
import tlsstream_model as SM
import tlsstreamcases as SC
from gopacket_amd import _lib, flows
from tlsstreamutil import HostChain, assert_same_streams, names_of, run_case_host
from tlsutil import assert_same_tls, model_and_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in SC.cases()}
MSG = SC.flight()
NREC = 3  # records of flight()


@pytest.mark.parametrize("name", list(CASES))
def test_host_matches_model(name):
    run_case_host(CASES[name], SC.PARSER)


def states(res):
    return [d["state"] for d in res]


def errs(d):
    return [(e["err"], e["status"]) for e in d["entries"]]


@pytest.mark.parametrize("two", [False, True], ids=["one_call", "two_calls"])
def test_every_split_position_gives_the_same_records(two):
    """One stream per cut position of a ClientHello, a CCS and an application
    record: each yields the same three records and the server name, whether
    the two segments come in one call or in two; the per-packet pass gives
    "TLS packet length mismatch" for the same packets."""
    calls = run_case_host(CASES["split_two_calls" if two else "split_one_call"], SC.PARSER)
    n = len(MSG) - 1
    got = {}
    for res in calls:
        assert len(res) == n and set(states(res)) == {SM.SYNCED}
        for d in res:
            got.setdefault(d["id"], []).extend((e["content_type"], e["length"], e["err"]) for e in d["entries"])
    want = [(22, len(SC.hello_rec()) - 5, 0), (20, 1, 0), (23, 40, 0)]
    assert all(got[g] == want for g in range(n)), [g for g in range(n) if got[g] != want][:5]
    assert sorted(x for res in calls for x in names_of(res)) == [(g, b"split.example") for g in range(n)]
    if two:  # tails of 1..4 bytes inside the header, and every later position
        assert [len(d["tail"]) for d in calls[0]] == [k if k < len(SC.hello_rec()) else
                                                      (k - len(SC.hello_rec()) if k < len(SC.hello_rec()) + 6 else
                                                       k - len(SC.hello_rec()) - 6) for k in range(1, n + 1)]
        assert all(d["tail_in"] == len(t["tail"]) for d, t in zip(calls[1], calls[0]))
    pk = [p for p in CASES["split_one_call"]["calls"][0] if len(p) > 54]
    m, h, _ = model_and_host(C.PARSER, pk)
    assert_same_tls(m, h)
    first = [int(m["records"][int(m["verdict"][i])]["err"]) for i in range(0, len(pk), 2)]
    assert first[4:len(SC.hello_rec()) - 1] == [M.E_LEN] * (len(SC.hello_rec()) - 5) and first[:4] == [M.E_REC_SHORT] * 4
    # a packet gives the name only where the cut falls on a record boundary: 2 of the streams, not all of them
    H = len(SC.hello_rec())
    assert M.snis(m) == [(2 * (H - 1), b"split.example"), (2 * (H + 6 - 1), b"split.example")]


def test_tail_is_bounded_by_the_16_bit_length():
    calls = run_case_host(CASES["largest_record"], SC.PARSER)
    assert [len(res[0]["tail"]) for res in calls] == [20 * SC.MSS, 65539, 0]
    assert _lib.TLSS_MAX_TAIL == SM.MAX_TAIL == 5 + 65535 - 1 == 65539
    assert [(e["content_type"], e["length"]) for e in calls[2][0]["entries"]] == [(23, 65535), (21, 2)]
    hdr = open(os.path.join(ROOT, "include", "gpk_tls_streams.h")).read()
    assert re.search(r"#define GPK_TLSS_MAX_TAIL 65539u", hdr)


def test_terminal_rules_by_hand():
    r = {n: run_case_host(CASES[n], SC.PARSER) for n in (
        "page_limit_forces_a_skip", "lost_middle_segment", "fin_inside_a_record", "no_syn", "no_syn_framed",
        "not_tls_is_sticky", "server_direction", "host_name_panic", "port_table", "out_of_order",
        "overlap_and_retransmission", "empty_records_300")}
    a, b = r["page_limit_forces_a_skip"]  # the records in front of the gap, one truncated entry, then nothing
    assert states(a) == [SM.LOST] and errs(a[0])[:3] == [(0, 0)] * 3 and errs(a[0])[-1] == (M.E_LEN, 1)
    assert states(b) == [SM.LOST] and b[0]["entries"] == [] and not b[0]["framed"]
    a, b = r["lost_middle_segment"]
    assert states(a) == [SM.SYNCED] and states(b) == [SM.LOST] and errs(b[0]) == [(M.E_LEN, 1)]
    (a,) = r["fin_inside_a_record"]
    assert states(a) == [SM.CLOSED] * 2 and errs(a[0])[-1] == (M.E_LEN, 1) and errs(a[1])[-1] == (M.E_REC_SHORT, 1)
    assert a[1]["entries"][-1]["content_type"] == 0 and len(a[0]["entries"]) == NREC + 1
    assert states(r["no_syn"][1]) == [SM.NOSTART] and r["no_syn"][1][0]["entries"] == []
    assert states(r["no_syn_framed"][1]) == [SM.CLOSED] and names_of(r["no_syn_framed"][1]) == [(0, b"nosyn.example")]
    a, b = r["not_tls_is_sticky"]
    assert states(a) == [SM.NOT_TLS] and errs(a[0]) == [(0, 0), (0, 0), (M.E_REC_TYPE, 0)]
    assert states(b) == [SM.NOT_TLS] and b[0]["entries"] == [] and a[0]["entries"][2]["content_type"] == ord("G")
    (a,) = r["server_direction"]
    assert errs(a[0]) == [(M.E_HS_TYPE, 0), (0, 0), (0, 0)] and states(a) == [SM.SYNCED]
    (a,) = r["host_name_panic"]
    assert errs(a[0]) == [(0, 0), (M.E_PANIC_SLICE_B, 0), (0, 0)]
    assert (a[0]["entries"][1]["err_a0"], a[0]["entries"][1]["err_a1"]) == (9, 1)
    (a,) = r["port_table"]
    assert states(a) == [SM.SYNCED, SM.NONE] and names_of(a) == [(0, b"alt.example")] and not a[1]["framed"]
    for n in ("out_of_order", "overlap_and_retransmission"):
        assert names_of(r[n][0]) == [(0, b"order.example")] and errs(r[n][0][0]) == [(0, 0)] * 4
    assert len(r["empty_records_300"][0][0]["entries"]) == 300


def test_buffer_ends_with_the_record():
    """The departure from the per-packet pass: a ClientHello cannot read into
    the next record. The per-packet pass decodes the spilling hello and its
    name; over streams the same bytes fail with "TLS ClientHello too short"."""
    spill = dict(C.quirk_cases()[0])["hello_spills_into_next_record"]
    m, h, _ = model_and_host(C.PARSER, [spill])
    assert M.snis(m) == [(0, b"spill.test")]
    case = dict(name="spill", calls=[SC.conn(1, spill[C.AT:], [3])], max_pages=0, frame_unstarted=False, flush=False)
    (res,) = run_case_host(case, SC.PARSER)
    assert errs(res[0]) == [(M.E_CH_SHORT, 1), (0, 0)] and names_of(res) == []


def test_quirk_streams_cover_every_error():
    (res,) = run_case_host(CASES["quirks"], SC.PARSER)
    seen = {e["err"] for d in res for e in d["entries"]}
    assert seen >= set(M.ALL_ERRORS) | {0}, set(M.ALL_ERRORS) - seen
    buf = ctypes.create_string_buffer(256)
    for d in res:  # the reference's texts
        for e in d["entries"]:
            n = _lib.lib().gpk_tls_format_error(e["err"], e["err_a0"], e["err_a1"], buf, 256)
            assert n == len(buf.value) and buf.value.decode() == M.error_text(e["err"], e["err_a0"], e["err_a1"])
    assert set(states(res)) == {SM.CLOSED, SM.NOT_TLS, SM.NONE}


@pytest.fixture(scope="module")
def mix():
    return SC.random_mix(20261021, 300)


def test_random_mix_in_three_calls(mix):
    case = dict(name="mix", calls=mix, max_pages=0, frame_unstarted=False, flush=True)
    calls = run_case_host(case, SC.PARSER)
    every = [d for res in calls for d in res]
    assert {d["state"] for d in every} >= {SM.SYNCED, SM.NONE, SM.NOSTART, SM.NOT_TLS, SM.LOST, SM.CLOSED}
    assert sum(len(d["tail"]) > 0 for d in every) > 50 and sum(d["tail_in"] > 0 and d["entries"] != [] for d in every) > 30
    assert len({x for res in calls for x in names_of(res)}) > 50


def one_call(pk, frame_unstarted=False):
    model = SM.Streaming(SC.PARSER, 0, frame_unstarted)
    model.feed(pk)
    return model.last


def test_capacity_rules():
    """Each arena in turn at exact and at exact - 1: a stream is written whole
    or not at all, nothing is written at or past a capacity, counts names the
    need, and the retry helper gets everything."""
    pk = [f for i in range(6) for f in SC.conn(i, SC.flight(b"cap%d.example" % i) + rec_tail(i), [70 + i])]
    last = one_call(pk)
    full, hfull = HostChain(SC.PARSER).call(last, keep=False)
    need = flows.TLSStreamDecoder.needed(hfull["counts"])
    assert need == tuple(len(full[k]) for k in ("recs", "hellos", "snis", "tails")) and min(need) > 0
    assert not int(hfull["counts"][5]) and not np.any(hfull["streams"][:6]["status"])
    for k in range(4):
        for caps in (need, tuple(x - (j == k) for j, x in enumerate(need)), tuple(0 if j == k else x for j, x in enumerate(need))):
            m, h = HostChain(SC.PARSER).call(last, caps=caps, keep=False)
            assert_same_streams(m, h, "caps %r" % (caps,))
            short = caps != need
            assert int(h["counts"][5]) == int(short) and flows.TLSStreamDecoder.needed(h["counts"]) == need
            st = h["streams"][:6]
            dropped = (st["status"] & _lib.TLSS_ST_DROPPED) != 0
            assert bool(dropped.any()) == short
            if short and caps[k] == need[k] - 1:  # only the last stream does not fit
                assert list(dropped) == [False] * 5 + [True]
            for t in st[~dropped]:  # what was kept is what the full run wrote
                a, b = int(t["rec0"]), int(t["rec0"]) + int(t["nrec"])
                assert b <= caps[0] and h["recs"][a:b].tobytes() == hfull["recs"][a:b].tobytes()
                a, b = int(t["tail_off"]), int(t["tail_off"]) + int(t["tail_len"])
                assert b <= caps[3] and h["tails"][a:b].tobytes() == hfull["tails"][a:b].tobytes()
            assert list(st["state"]) == list(hfull["streams"][:6]["state"])  # state and sizes are set all the same
    data, off, cap, ref = last["arrays"]
    out = flows.TLSStreamDecoder.decode_host_all(HostChain(SC.PARSER).parser, data, off, cap, ref["records"],
                                                 ref["layouts"], SM.asm_arrays(last["asm"], len(cap)))
    assert not int(out["counts"][5])
    for k in ("recs", "hellos", "snis", "tails"):
        assert out[k].tobytes() == hfull[k].tobytes(), k


def rec_tail(i):
    return C.rec(C.APP, bytes(50))[:7 + i]  # an unfinished record: a tail of 7 + i bytes


def test_toobig_is_lost_without_reading_a_byte():
    """A forged stream_data0 with no bytes behind it: a logical buffer of 2^32
    bytes or more is TOOBIG and treated as LOST; so is a stream past data_cap."""
    last = one_call(SC.conn(1, SC.flight(), [50]) + SC.conn(2, SC.flight(), [60]))
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
        h = flows.TLSStreamDecoder.decode_host(p, data, off, cap, ref["records"], ref["layouts"], a, 8, 8, 64, 64)
        st = h["streams"][:2]
        assert list(st["state"]) == want, forged
        big = st[st["state"] == SM.LOST][0]
        assert int(big["status"]) == _lib.TLSS_ST_TOOBIG and int(big["nrec"]) == 0 and int(big["tail_len"]) == 0
        assert int(h["counts"][0]) == 2 and int(h["counts"][1]) == 2
    # a tail that does not lie in the arena
    a = dict(asm)
    carry = (np.array([SM.SYNCED, SM.SYNCED], np.uint32), np.array([0, 6], np.uint64), np.array([4, 5], np.uint32),
             np.zeros(10, np.uint8))
    h = flows.TLSStreamDecoder.decode_host(p, data, off, cap, ref["records"], ref["layouts"], a, 8, 8, 64, 64, carry=carry)
    assert [int(x) for x in h["streams"][:2]["status"]] == [0, _lib.TLSS_ST_BADTAIL]
    assert [int(x) for x in h["streams"][:2]["state"]] == [SM.NOT_TLS, SM.LOST]  # four zero bytes in front: no TLS


def test_host_argument_checks():
    last = one_call(SC.conn(1, SC.flight(), [50]))
    data, off, cap, ref = last["arrays"]
    n = len(cap)
    p = HostChain(SC.PARSER).parser
    asm = SM.asm_arrays(last["asm"], n)
    good = flows.TLSStreamDecoder.decode_host(p, data, off, cap, ref["records"], ref["layouts"], asm, 8, 4, 64, 64)
    assert flows.TLSStreamDecoder.needed(good["counts"]) == (3, 1, 13, 0) and list(good["counts"][:6]) == [1, 1, 3, 0, 1, 0]
    lib = _lib.lib()
    b = _lib.Batch(data.ctypes.data, off.ctypes.data, cap.ctypes.data, n, data.size)
    r = _lib.Results(ref["records"].ctypes.data, None, None, ref["layouts"].ctypes.data)
    keys = flows.TLSStreamDecoder.ASM_KEYS

    def call(parser=p, batch=b, inp=None, asm_kw=(), **kw):
        av = {k: asm[k].ctypes.data if k in asm else None for k in keys}
        av.update(asm_kw)
        a = _lib.TcpStreams(*[av[k] for k in keys], asm["chunk_cap"], asm["data_cap"])
        o = dict(streams=good["streams"].ctypes.data, recs=good["recs"].ctypes.data, hellos=good["hellos"].ctypes.data,
                 snis=good["snis"].ctypes.data, tails=good["tails"].ctypes.data, counts=good["counts"].ctypes.data,
                 rec_cap=8, hello_cap=4, sni_cap=64, tail_cap=64)
        o.update(kw)
        return lib.gpk_tls_streams_host(parser.h if parser else None, ctypes.byref(batch), ctypes.byref(r), ctypes.byref(a),
                                        ctypes.byref(inp) if inp is not None else None, ctypes.byref(_lib.TlsStreamOut(**o)))
    assert call() == 0
    odd = good["recs"].ctypes.data + 4
    for kw in (dict(streams=None), dict(counts=None), dict(recs=None), dict(hellos=None), dict(snis=None),
               dict(tails=None), dict(recs=odd), dict(hellos=odd), dict(streams=good["streams"].ctypes.data + 4),
               dict(asm_kw=dict(counts=None)), dict(asm_kw=dict(chunks=None)), dict(asm_kw=dict(stream_first=None)),
               dict(asm_kw=dict(stream_closed=None)), dict(asm_kw=dict(stream_data0=None)), dict(asm_kw=dict(data=None)),
               dict(parser=None)):
        assert call(**kw) == _lib.GPK_EINVAL, kw
    assert call(recs=None, rec_cap=0) == 0 and call(hellos=None, hello_cap=0) == 0 and call(snis=None, sni_cap=0) == 0
    assert call(tails=None, tail_cap=0) == 0
    st = np.zeros(n + 1, np.uint32)
    z8, z4 = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
    mk = lambda **kw: _lib.TlsStreamIn(**dict(dict(state=st.ctypes.data, tail_off=z8.ctypes.data,  # noqa: E731
                                                    tail_len=z4.ctypes.data, tails=None, n=1, tail_bytes=0, flags=0), **kw))
    assert call(inp=mk()) == 0 and call(inp=mk(flags=_lib.TLSS_FRAME_UNSTARTED)) == 0
    for bad in (mk(flags=2), mk(n=n + 1), mk(state=None), mk(tail_off=None), mk(tail_len=None), mk(tail_bytes=4)):
        assert call(inp=bad) == _lib.GPK_EINVAL
    empty = _lib.Batch(None, None, None, 0, 0)
    assert call(batch=empty) == 0 and list(good["counts"]) == [0] * 12


def test_abi_layout_of_tls_stream_structs(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler (gcc, cc or clang): the build needs a host compiler too"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_tls_streams.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_tls_stream", _lib.TLS_STREAM_DTYPE), ("gpk_tls_stream_rec", _lib.TLS_STREAM_REC_DTYPE),
                          ("gpk_tls_stream_in", _lib.TlsStreamIn), ("gpk_tls_stream_out", _lib.TlsStreamOut)):
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
    assert (_lib.TLS_STREAM_DTYPE.itemsize, _lib.TLS_STREAM_REC_DTYPE.itemsize) == (64, 32)
    assert _lib.TLS_STREAM_REC_DTYPE.fields["rec"][0] == _lib.TLS_REC_DTYPE  # the first 16 bytes, unchanged


def test_exports_and_constants():
    for name in ("gpk_tls_stream_decoder_create", "gpk_tls_stream_decoder_destroy", "gpk_tls_streams",
                 "gpk_tls_streams_host"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "gpk_tls_streams.h")).read()
    for cname, val in (("GPK_TLSS_NEW", _lib.TLSS_NEW), ("GPK_TLSS_SYNCED", _lib.TLSS_SYNCED),
                       ("GPK_TLSS_NONE", _lib.TLSS_NONE), ("GPK_TLSS_NOSTART", _lib.TLSS_NOSTART),
                       ("GPK_TLSS_NOT_TLS", _lib.TLSS_NOT_TLS), ("GPK_TLSS_LOST", _lib.TLSS_LOST),
                       ("GPK_TLSS_CLOSED", _lib.TLSS_CLOSED), ("GPK_TLSS_NSTATE", _lib.TLSS_NSTATE),
                       ("GPK_TLSS_ST_DROPPED", _lib.TLSS_ST_DROPPED), ("GPK_TLSS_ST_TOOBIG", _lib.TLSS_ST_TOOBIG),
                       ("GPK_TLSS_ST_BADTAIL", _lib.TLSS_ST_BADTAIL),
                       ("GPK_TLSS_FRAME_UNSTARTED", _lib.TLSS_FRAME_UNSTARTED), ("GPK_TLSS_MAX_TAIL", _lib.TLSS_MAX_TAIL)):
        assert re.search(r"#define %s %su?\s" % (cname, val), hdr), cname
    assert (SM.NEW, SM.SYNCED, SM.NONE, SM.NOSTART, SM.NOT_TLS, SM.LOST, SM.CLOSED) == tuple(range(7))
    assert _lib.TLS_ERR_END - _lib.TLS_ERR_FIRST == 12  # no error code was added
    for cls in (flows.TLSStreamDecoder, flows.TLSStreams):
        assert cls.__doc__
    for name in ("decode", "decode_all", "decode_host", "decode_host_all"):
        assert callable(getattr(flows.TLSStreamDecoder, name))
    for name in ("feed", "flush_all", "flush_older_than"):
        assert callable(getattr(flows.TLSStreams, name))


def test_per_packet_pass_is_unchanged():
    """The walk's loop body became a shared function: the per-packet pass still
    equals its model on the hand-built cases and on the seeded corpus."""
    cases = [p for _, p in C.quirk_cases()[0]]
    m, h, _ = model_and_host(C.PARSER, cases, fill=0xA5)
    assert_same_tls(m, h, "cases")
    m, h, _ = model_and_host(C.PARSER, C.fuzz_packets(C.FUZZ_SEED, 1024), align=16, pad=3, fill=0xA5)
    assert_same_tls(m, h, "fuzz")
    assert int(m["counts"][1]) > 100 and int(m["counts"][2]) > 100
