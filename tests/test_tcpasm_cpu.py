"""The TCP reassembly model (tests/tcpasm_model.py) pinned on tcpassembly's own
tests (assembly_test.go:27-467): real Ethernet/IPv4/TCP frames built from each
layers.TCP{Seq, SYN, Payload}, netFlow 1.2.3.4->5.6.7.8, ports 1->2,
MaxBufferedPagesPerConnection = 4, and the chunks delivered per call compared
with `want` (Bytes, Skip, Start, End). Model-only properties on random
traffic. Plus the C side of include/gpk_tcpasm.h: it compiles as C11 and C++,
and its structs and constants match gopacket_amd/_lib.py. CPU only; the device
path is tests/test_tcpasm_gpu.py."""
import ctypes
import functools
import json
import os
import shutil
import subprocess

import pytest

import flowcases
import pktutil
import tcpasm_model as M
import tcpasmcases as TC
from configs import oracle_parser
from gopacket_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = flowcases.DEFRAG_PARSER


def run_model(packets, **kw):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(CFG).decode(data, off, cap, layouts=True)
    r = M.run(packets, res["records"], res["layouts"], **kw)
    r["layouts"] = res["layouts"]
    return r


def delivered(r, call):
    """The Reassembly list of Assemble call `call`: (Bytes, Skip, Start, End)."""
    out = []
    for st in r["streams"]:
        at = 0
        for ch in st["chunks"]:
            if ch["call"] == call:
                out.append((st["data"][at:at + ch["len"]], ch["skip"], bool(ch["flags"] & M.START),
                            bool(ch["flags"] & M.END)))
            at += ch["len"]
    return out


def test_sequence_overflow():
    """TestSequenceOverflow (:27-31)"""
    assert M.difference(2 ** 32 - 10, 10) == 20
    assert M.difference(4, 8) == 4 and M.difference(8, 4) == -4  # :51-52
    assert M.add(2 ** 32 - 1, 2) == 1


@pytest.mark.parametrize("name", sorted(TC.REFERENCE))
def test_reference_sequences(name):
    r = run_model(TC.reference_packets(name), max_pages=4)
    assert r["counts"][0] == 1 and set(r["stream_of"]) == {0}
    for i, (_, _, _, want) in enumerate(TC.REFERENCE[name]):
        assert delivered(r, i) == want, (name, i)
        assert r["verdict"][i] in (M.DIRECT, M.QUEUED)


def test_quirks_by_hand():
    S, F = TC.SYN, TC.FIN
    # a retransmitted SYN and an old retransmission deliver an empty chunk, nextSeq unchanged (:619-621)
    r = run_model([TC.seg(100, S), TC.seg(100, S), TC.seg(101, 0, b"abcd"), TC.seg(101, 0, b"ab"),
                   TC.seg(105, F)])
    assert [(c["len"], c["flags"]) for c in r["streams"][0]["chunks"]] == [(0, M.START), (0, 0), (4, 0), (0, 0),
                                                                           (0, M.END)]
    assert r["streams"][0]["closed"] == 4 and r["conn_seq"] == [M.NO_CONN]
    # a bare FIN on an unknown key creates nothing (:555-560); data after a FIN makes a new instance
    r = run_model([TC.seg(5, F), TC.seg(9, S, b"x"), TC.seg(11, F), TC.seg(12, 0, b"late")], flush=True)
    assert r["verdict"] == [M.NOCONN, M.DIRECT, M.DIRECT, M.QUEUED] and r["counts"][0] == 2
    assert r["streams"][1]["chunks"][0]["skip"] == -1 and r["streams"][1]["closed"] == M.CALL_FLUSH | 1
    # an End page that is not the last of ret does not close (:633)
    r = run_model([TC.seg(10, S), TC.seg(13, F, b"cd"), TC.seg(15, 0, b"ef"), TC.seg(11, 0, b"ab")])
    assert [c["flags"] for c in r["streams"][0]["chunks"]] == [M.START, 0, M.END, 0]
    assert r["streams"][0]["closed"] == M.OPEN and r["conn_seq"] == [17]
    # the first SYN's chunk has no End even with FIN set (:576-581): the connection stays open
    r = run_model([TC.seg(10, S | F, b"zz")])
    assert r["streams"][0]["chunks"][0]["flags"] == M.START and r["conn_seq"] == [13]
    # Skip past 2^31 (:766-767)
    r = run_model([TC.seg(0, S), TC.seg(2 ** 31 + 5, 0, b"q")], flush=True)
    assert r["streams"][0]["chunks"][1]["skip"] == 2 ** 31 + 4


@functools.lru_cache(maxsize=None)
def random_case():
    pk = TC.random_traffic(3, 600)
    return pk, {(mp, fl): run_model(pk, max_pages=mp, flush=fl) for mp in (0, 4) for fl in (False, True)}


@pytest.mark.parametrize("mp,fl", [(0, False), (0, True), (4, False), (4, True)])
def test_random_traffic_properties(mp, fl):
    pk, runs = random_case()
    r = runs[(mp, fl)]
    assert r["counts"][0] > 600 and M.QUEUED in r["verdict"] and M.NOCONN in r["verdict"]
    assert fl or r["counts"][3] > 0
    for st in r["streams"]:
        prev_end, at = None, 0
        for ch in st["chunks"]:
            sg = M.Seg(ch["src"], pk[ch["src"]], r["layouts"][ch["src"]])
            # every chunk's bytes equal the source payload slice
            lo = sg.pstart + ch["src_off"]
            assert st["data"][at:at + ch["len"]] == pk[ch["src"]][lo:lo + ch["len"]]
            assert ch["src_off"] + ch["len"] <= sg.plen
            at += ch["len"]
            if ch["len"] == 0:
                continue
            # ranges ascend without overlap in Difference order; a SYN takes one sequence number
            first = M.add(sg.seq, ch["src_off"] + (1 if ch["flags"] & M.START else 0))
            if prev_end is not None:
                assert M.difference(prev_end, first) >= 0, (st["first"], ch)
                assert (M.difference(prev_end, first) > 0) == (ch["skip"] > 0)
            prev_end = M.add(first, ch["len"])
        assert at == len(st["data"])


def test_carry_reproduces_the_state():
    """Cutting a sequence in two and feeding conn_seq / first / pend back as
    carried entries gives the chunks of the one-batch run, a partly popped
    multi-page packet included."""
    S = TC.SYN
    pk = [TC.seg(1000, S), TC.seg(1001 + 100, 0, bytes(range(256)) * 20), TC.seg(1001, 0, b"a" * 60),
          TC.seg(1001 + 100 + 5120, TC.FIN, b"end")]
    whole = run_model(pk, max_pages=2, flush=True)
    for cut in range(len(pk) + 1):
        a = run_model(pk[:cut], max_pages=2)
        carry_pk, carry = [], []
        groups = _group_first(pk[:cut])
        for g, seq in enumerate(a["conn_seq"]):
            if seq == M.NO_CONN:
                continue
            carry_pk.append(groups[g])
            carry.append((M.CARRY_CONN, seq))
            for p, k in a["pend"]:  # one key in this test
                carry_pk.append(p)
                carry.append((M.CARRY_PAGE | k, 0))
        b = run_model([pk[i] for i in carry_pk] + pk[cut:], max_pages=2, flush=True, carry=carry)
        origin = carry_pk + list(range(cut, len(pk)))
        got = [(org[c["src"]], c["src_off"], c["len"], c["skip"], c["flags"])
               for r_, org in ((a, list(range(cut))), (b, origin)) for st in r_["streams"] for c in st["chunks"]]
        want = [(c["src"], c["src_off"], c["len"], c["skip"], c["flags"]) for st in whole["streams"]
                for c in st["chunks"]]
        assert got == want, cut
    # addContiguous always takes the pages behind a popped page 0 (each starts where its
    # predecessor ends), so traffic leaves no packet partly popped between two calls; the
    # carried form can still state it: pages 1 and 2 of packet 1 without page 0
    r = run_model([pk[0], pk[1], pk[1]], flush=True,
                  carry=[(M.CARRY_CONN, 1001), (M.CARRY_PAGE | 1, 0), (M.CARRY_PAGE | 2, 0)])
    assert [(c["src"], c["src_off"], c["len"], c["skip"]) for c in r["streams"][0]["chunks"]] == \
        [(1, 1900, 1900, 2000), (2, 3800, 1320, 0)]
    assert r["verdict"] == [M.CARRIED] * 3
    r = run_model([pk[1], pk[0]], carry=[(M.CARRY_PAGE | 1, 0), (M.CARRY_CONN | M.CARRY_PAGE, 0)])
    assert r["verdict"] == [M.EBADCARRY] * 2 and r["counts"][0] == 0


def _decode(packets):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(CFG).decode(data, off, cap, layouts=True)
    return res["records"], res["layouts"]


def _group_first(packets):
    from oracle import flows_oracle as FO
    rec, lay = _decode(packets) if packets else ([], [])
    first = []
    seen = set()
    for i, p in enumerate(packets):
        k = FO.packet_key(FO.CONNECTION, p, rec[i], lay[i], 0, 8)
        if not isinstance(k, int) and k not in seen:
            seen.add(k)
            first.append(i)
    return first


def test_header_compiles_as_c11_and_cxx(tmp_path):
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if not shutil.which(cc):
            pytest.skip("needs " + cc)
        src = tmp_path / ("hdr." + ext)
        src.write_text('#include "gpk_tcpasm.h"\nint main(void) { gpk_tcp_streams s; gpk_tcpasm_opts o; gpk_tcp_chunk c; '
                       '(void)s; (void)o; (void)c; return GPK_TCPASM_DIRECT + 24; }\n')
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                            str(tmp_path / "hdr.o"), str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_structs_and_constants_match_python(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    structs = dict(gpk_tcp_streams=_lib.TcpStreams, gpk_tcpasm_opts=_lib.TcpasmOpts)
    consts = dict(GPK_TCPASM_DIRECT=_lib.TCPASM_DIRECT, GPK_TCPASM_QUEUED=_lib.TCPASM_QUEUED,
                  GPK_TCPASM_NOCONN=_lib.TCPASM_NOCONN, GPK_TCPASM_CARRIED=_lib.TCPASM_CARRIED,
                  GPK_TCPASM_EBADCARRY=_lib.TCPASM_EBADCARRY, GPK_TCPASM_EPANIC=_lib.TCPASM_EPANIC,
                  GPK_TCPASM_PAGE_BYTES=_lib.TCPASM_PAGE_BYTES, GPK_TCP_START=_lib.TCP_START, GPK_TCP_END=_lib.TCP_END,
                  GPK_TCPASM_CALL_FLUSH=_lib.TCPASM_CALL_FLUSH, GPK_TCPASM_OPEN=_lib.TCPASM_OPEN,
                  GPK_TCPASM_NO_CONN=_lib.TCPASM_NO_CONN, GPK_TCPASM_CARRY_CONN=_lib.TCPASM_CARRY_CONN,
                  GPK_TCPASM_CARRY_PAGE=_lib.TCPASM_CARRY_PAGE)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gpk_tcpasm.h"', "int main(void) {", '  printf("{");']
    for s, cls in structs.items():
        lines.append('  printf("\\"%s\\": %%zu, ", sizeof(%s));' % (s, s))
        lines += ['  printf("\\"%s.%s\\": %%zu, ", offsetof(%s, %s));' % (s, f, s, f) for f, _ in cls._fields_]
    lines.append('  printf("\\"gpk_tcp_chunk\\": %zu, ", sizeof(gpk_tcp_chunk));')
    lines += ['  printf("\\"gpk_tcp_chunk.%s\\": %%zu, ", offsetof(gpk_tcp_chunk, %s));' % (f, f)
              for f in _lib.TCP_CHUNK_DTYPE.names]
    lines += ['  printf("\\"%s\\": %%lld, ", (long long)%s);' % (c, c) for c in consts]
    lines += ['  printf("\\"end\\": 0}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout)
    for s, cls in structs.items():
        assert got[s] == ctypes.sizeof(cls), s
        for f, _ in cls._fields_:
            assert got["%s.%s" % (s, f)] == getattr(cls, f).offset, (s, f)
    assert got["gpk_tcp_chunk"] == _lib.TCP_CHUNK_DTYPE.itemsize == 40
    for f in _lib.TCP_CHUNK_DTYPE.names:
        assert got["gpk_tcp_chunk." + f] == _lib.TCP_CHUNK_DTYPE.fields[f][1], f
    for c, v in consts.items():
        assert got[c] == v, c
    for name in ("DIRECT", "QUEUED", "NOCONN", "CARRIED", "EBADCARRY", "EPANIC", "CALL_FLUSH", "OPEN", "NO_CONN",
                 "CARRY_CONN", "CARRY_PAGE"):
        assert getattr(M, name) == getattr(_lib, "TCPASM_" + name), name
    assert (M.START, M.END, M.PAGE_BYTES) == (_lib.TCP_START, _lib.TCP_END, _lib.TCPASM_PAGE_BYTES)
