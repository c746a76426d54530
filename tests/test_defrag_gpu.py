"""gpk_defrag_batch (IPv4 reassembly in HBM, include/gpk_defrag.h) against the
reassembly model (tests/defrag_model.py) run on the decode oracle's results:
the same verdict for every packet, the same datagrams in the same order
(last, length, payload_off, every byte), the same pending list and counts.
No tolerance anywhere."""
import functools

import numpy as np
import pytest

import defrag_model as M
import defragcases as DC
import flowcases
import pktutil
from configs import device_parser, oracle_parser
from gopacket_amd import _lib, flows
from oracle import flows_oracle as FO
from test_defrag_cpu import SEQUENCES

pytestmark = pytest.mark.gpu

CFG = flowcases.DEFRAG_PARSER


def upload(packets):
    import torch
    data, off, cap = pktutil.pack(packets)
    return (data, off, cap), (torch.from_numpy(data).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                              torch.from_numpy(cap.astype(np.int32)).cuda())


def device_decode(gpu_ctx, d, o, c, cfg=CFG):
    import torch
    n = max(o.numel(), 1)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(device_parser(cfg), d, o, c, rec, None, fl, lay, stream=torch.cuda.current_stream())
    return rec, lay


def model(packets):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(CFG).decode(data, off, cap, layouts=True)
    return M.run(packets, res["records"], res["layouts"])


def device_defrag(gpu_ctx, packets, data_cap=None, guard=0):
    """-> (host dict: verdict, last, length, payload_off, offsets, caplens, pending, counts, data; device dict)"""
    import torch
    _, (d, o, c) = upload(packets)
    rec, lay = device_decode(gpu_ctx, d, o, c)
    n = len(packets)
    g = flows.Grouper(max(n, 1))
    df = flows.Defragmenter(max(n, 1))
    groups = g.group(d, o, c, rec, lay, kind=FO.DEFRAG)
    out_data = None
    if data_cap is not None:
        out_data = torch.full((data_cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = df.defrag(d, o, c, rec, lay, groups, data_cap=data_cap, out_data=out_data)
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    D, P = counts[0], counts[1]
    host = dict(verdict=out["verdict"].cpu().tolist(), counts=counts, pending=out["pending"][:P].cpu().tolist(),
                data=out["data"].cpu().numpy())
    for k in ("last", "length", "payload_off", "offsets", "caplens"):
        host[k] = out[k][:D].cpu().tolist()
    g.close()
    df.close()
    return host, out


def check(gpu_ctx, packets, ref=None):
    ref = ref or model(packets)
    got, out = device_defrag(gpu_ctx, packets)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got["verdict"], ref["verdict"])) if a != b]
    assert not bad and len(got["verdict"]) == len(ref["verdict"]), bad[:8]
    dg = ref["datagrams"]
    assert got["last"] == [d["last"] for d in dg]
    assert got["length"] == [d["length"] for d in dg]
    assert got["payload_off"] == [d["payload_off"] for d in dg]
    assert got["caplens"] == [len(d["data"]) for d in dg]
    assert got["offsets"] == [int(x) for x in np.cumsum([0] + [len(d["data"]) for d in dg])[:-1]]
    blob = got["data"]
    for j, d in enumerate(dg):
        mine = blob[got["offsets"][j]:got["offsets"][j] + got["caplens"][j]].tobytes()
        assert mine == d["data"], ("datagram", j, next(k for k in range(len(mine)) if mine[k] != d["data"][k]))
        assert mine[d["payload_off"]:] == d["payload"]
    assert got["pending"] == ref["pending"]
    assert got["counts"] == [len(dg), len(ref["pending"]), sum(len(d["data"]) for d in dg), 0]
    return ref, got, out


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_reference_sequences(gpu_ctx, name):
    frames, _ = flowcases.defrag_frames()
    order, expect = SEQUENCES[name]
    ref, got, _ = check(gpu_ctx, [frames[k] for k in order])
    assert [v >= 0 for v in got["verdict"]] == expect


def test_struct_cases(gpu_ctx):
    check(gpu_ctx, [f for _, f in flowcases.defrag_struct_cases()])


FIRST = (8, 16, 24, 1480)
FINAL = (0, 1, 7, 8, 15, 16, 17, 1479)
HEADERS = {"plain": {}, "vlan": dict(vlan=5), "ihl6": dict(ihl=6), "ihl15": dict(ihl=15)}


@pytest.mark.parametrize("hdr", sorted(HEADERS))
def test_alignment_and_size_sweep(gpu_ctx, hdr):
    """Two-fragment datagrams, every first/final size, each behind 0-15 junk
    packets of odd length, so the source and destination 16-byte phases take
    all their values; Ethernet padding after a short final fragment. The
    options sit on the final fragment, the one whose header the datagram gets:
    fragLength is Length - 20 whatever the IHL, so a first fragment with
    options never lines up with the next offset in the reference (those
    sequences are compared too, and yield no datagram)."""
    rng = np.random.default_rng(5)
    pk, ident = [], 0
    for junk in range(16):
        for a in FIRST:
            for b in FINAL:
                pk += [DC.body(rng, 2 * j + 1 + junk) for j in range(junk)]
                ident += 1
                first = {k: v for k, v in HEADERS[hdr].items() if k == "vlan"}
                pk.append(DC.frag(ident, 0, 1, DC.body(rng, a), **first))
                pk.append(DC.frag(ident, a // 8, 0, DC.body(rng, b), pad=(46 - b if b < 18 and junk & 1 else 0),
                                  **HEADERS[hdr]))
    ref, got, _ = check(gpu_ctx, pk)
    assert len(ref["datagrams"]) == 16 * len(FIRST) * len(FINAL)
    assert {o & 15 for o in got["offsets"]} == set(range(16))
    if "ihl" in HEADERS[hdr]:  # options on every fragment: held for ever, as in the reference
        pk = [DC.frag(1, 0, 1, DC.body(rng, 24), **HEADERS[hdr]), DC.frag(1, 3, 0, DC.body(rng, 9), **HEADERS[hdr])]
        ref, _, _ = check(gpu_ctx, pk)
        assert ref["verdict"] == [M.HELD, M.HELD]


def in_order(ident, k, rng, per=8):
    return [DC.frag(ident, j * per // 8, 1 if j + 1 < k else 0, DC.body(rng, per if j + 1 < k else 5))
            for j in range(k)]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 129])
def test_group_sizes_around_the_wave(gpu_ctx, k):
    rng = np.random.default_rng(k)
    fwd = in_order(1, k, rng)
    if k == 1:  # a lone first fragment: held
        fwd = [DC.frag(1, 0, 1, DC.body(rng, 8))]
    rev = in_order(2, k, rng)[::-1] if k > 1 else [DC.frag(2, 3, 0, DC.body(rng, 8))]
    ref, _, _ = check(gpu_ctx, fwd + rev)
    assert len(ref["datagrams"]) == (2 if k > 1 else 0)


def test_interleaved_keys_and_repeated_completion(gpu_ctx):
    rng = np.random.default_rng(11)
    keys = [in_order(100 + q, 5, rng, per=24) for q in range(64)]
    pk = [keys[q][j] for j in range(5) for q in range(64)]       # 64 keys round-robin
    one = in_order(7, 4, rng, per=16)
    pk += one + one[::-1] + [one[0], one[2], one[1], one[3]]     # one key completing three times
    ref, _, _ = check(gpu_ctx, pk)
    assert len(ref["datagrams"]) == 64 + 3


@pytest.mark.parametrize("name", sorted(DC.quirk_cases()))
def test_quirks(gpu_ctx, name):
    pk, verdict, pending = DC.quirk_cases()[name]
    ref, got, _ = check(gpu_ctx, pk)
    assert got["verdict"] == verdict and got["pending"] == pending


def test_maximum_list_length(gpu_ctx):
    """8192 copies of an MF fragment at FragOffset 8183: every copy is pushed,
    the 8192nd flushes the key; one more starts a new list. Then a long key
    whose fragments arrive reversed (every insert shifts the whole list)."""
    f = DC.frag(9, 8183, 1, b"c" * 80)
    rng = np.random.default_rng(2)
    pk = [f] * (M.MAX_LIST + 1) + in_order(10, 700, rng)[::-1]
    ref, got, _ = check(gpu_ctx, pk)
    assert got["verdict"][M.MAX_LIST - 1] == M.EMAXLEN and got["pending"] == [M.MAX_LIST]
    assert len(ref["datagrams"]) == 1


@functools.lru_cache(maxsize=None)
def random_case():
    pk = DC.random_traffic(4, 3000, lo=2500, hi=7000, per=744)
    return pk, model(pk)


def test_random_traffic(gpu_ctx):
    pk, ref = random_case()
    v = ref["verdict"]
    assert 19000 < len(pk) < 23000
    assert len(ref["datagrams"]) >= 1500 and M.HELD in v and M.EHOLE in v
    assert any(c in v for c in (FO.FRAG_TOO_SMALL, FO.FRAG_OFFSET))
    check(gpu_ctx, pk, ref)


def test_fuzz_packets_do_not_fault(gpu_ctx):
    pk = pktutil.fuzz_packets(91, 20000)
    check(gpu_ctx, pk)


def test_edges(gpu_ctx):
    check(gpu_ctx, [flowcases.connection_cases()[0], b"\x00" * 10])   # no keyed packet
    check(gpu_ctx, [DC.frag(1, 0, 1, b"a" * 8), DC.frag(2, 0, 1, b"b" * 8)])  # keyed, no datagram
    import torch
    df = flows.Defragmenter(4)
    z64, z32, z8 = (torch.zeros(1, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.uint8))
    groups = dict(group_of=z32, perm=z32, start=z32, first=z32, counts=torch.zeros(2, dtype=torch.int32, device="cuda"))
    out = df.defrag(z8, z64[:0], z32[:0], z8, z8, groups)
    torch.cuda.synchronize()
    assert out["counts"].cpu().tolist() == [0, 0, 0, 0]
    df.close()


def test_data_cap_overflow(gpu_ctx):
    """data_cap too small: the flag is set, the needed bytes are right, nothing
    is written past the cap (a guard region stays untouched), and the datagrams
    that fit are whole."""
    rng = np.random.default_rng(8)
    pk = []
    for q in range(6):
        pk += DC.fragments(q, DC.body(rng, 900 + q), per=304)
    ref = model(pk)
    sizes = [len(d["data"]) for d in ref["datagrams"]]
    need = sum(sizes)
    cap = sum(sizes[:3]) + 77          # ends inside the fourth datagram
    got, _ = device_defrag(gpu_ctx, pk, data_cap=cap, guard=4096)
    assert got["counts"] == [6, 0, need, 1]
    blob = got["data"]
    assert np.all(blob[sum(sizes[:3]):] == 0xA5)
    for j in range(3):
        assert blob[got["offsets"][j]:got["offsets"][j] + sizes[j]].tobytes() == ref["datagrams"][j]["data"]
    assert got["verdict"] == ref["verdict"] and got["caplens"] == sizes


def test_streaming_two_batches(gpu_ctx):
    """TestDefragPing1and2's sequence with Ping1 appended again, cut in two at
    every position: the same datagrams in the same order as from one batch."""
    import torch
    frames, _ = flowcases.defrag_frames()
    order = SEQUENCES["TestDefragPing1and2"][0] + SEQUENCES["TestDefragIDField"][0]
    pk = [frames[k] for k in order]
    whole = model(pk)
    assert len(whole["datagrams"]) == 3
    s = flows.IPv4Defragmenter(gpu_ctx, device_parser(CFG), 64)
    for cut in range(len(pk) + 1):
        seen, verdicts = [], []
        for part in (pk[:cut], pk[cut:]):
            _, (d, o, c) = upload(part)
            out = s.defrag(d, o[:len(part)], c[:len(part)])
            torch.cuda.synchronize()
            blob = out["data"].cpu().numpy()
            for j in range(out["datagrams"]):
                at, ln = int(out["offsets"][j]), int(out["caplens"][j])
                seen.append((len(verdicts) + int(out["last"][j]), int(out["length"][j]), blob[at:at + ln].tobytes()))
            verdicts += [v if v < 0 else v + len(seen) - out["datagrams"] for v in out["verdict"].cpu().tolist()]
            if len(verdicts) == cut:  # after the first batch
                assert s.pending_count == len(model(pk[:cut])["pending"])
        assert seen == [(d["last"], d["length"], d["data"]) for d in whole["datagrams"]], cut
        assert verdicts == whole["verdict"], cut
        assert s.pending_count == len(whole["pending"]) == 0
    _, (d, o, c) = upload(pk[:3])
    s.defrag(d, o, c)
    assert s.pending_count == 3 and s.flush() == 3 and s.pending_count == 0
    s.close()


def test_redecode_datagrams(gpu_ctx):
    """The datagram batch decodes again with the statsassembly parser: records
    equal the decode oracle's on the same bytes, and a UDP datagram built with a
    correct checksum verifies over the whole reassembled payload."""
    import torch
    rng = np.random.default_rng(21)
    pk = []
    for q in range(40):
        src, dst = (10, 9, 0, 1 + q), (10, 9, 1, 7)
        l4 = DC.udp_segment(src, dst, 5000 + q, 6000, DC.body(rng, 300 + 97 * q))
        fr = DC.fragments(q, l4, 256, src, dst, **({"vlan": 9} if q & 1 else {}))
        pk += fr[::-1] if q % 3 == 0 else fr
    ref, got, out = check(gpu_ctx, pk)
    D = got["counts"][0]
    assert D == 40
    dd, do, dc = out["data"], out["offsets"][:D].contiguous(), out["caplens"][:D].contiguous()
    cfg = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"])
    rec, _ = device_decode(gpu_ctx, dd, do, dc, cfg)
    torch.cuda.synchronize()
    recs = rec.cpu().numpy().view(_lib.RECORD_DTYPE)[:D]
    want = oracle_parser(cfg).decode(got["data"], np.array(got["offsets"], np.uint64),
                                     np.array(got["caplens"], np.uint32), layouts=True)["records"]
    for f in ("layers", "status", "ip4_csum", "l4_csum"):
        assert np.array_equal(recs[f], want[f]), f
    ok = (1 << 22) | (1 << 23) | (1 << 24)  # GPK_ST_L4_CSUM | GPK_ST_L4_VALID | GPK_ST_L4_UDP
    assert np.all(recs["status"] & ok == ok) and np.all(recs["status"] & 0x7F == 0)
    assert np.all(recs["status"] & ((1 << 20) | (1 << 21)) == (1 << 20) | (1 << 21))  # the recomputed IPv4 checksum


def test_jumbo_fragments_and_total_length_past_16_bits(gpu_ctx):
    """Fragments of tens of kilobytes (many 16-byte store rounds per wave), and
    a datagram whose header + payload exceed 65535: Total Length is written as
    0, which DecodeFromBytes reads as the slice's length."""
    rng = np.random.default_rng(13)
    pk = [b"\x01" * 3,
          DC.frag(1, 0, 1, DC.body(rng, 40000)), DC.frag(1, 5000, 0, DC.body(rng, 20001)),
          DC.frag(2, 5000, 0, DC.body(rng, 25530)), DC.frag(2, 0, 1, DC.body(rng, 40000))]
    ref, got, _ = check(gpu_ctx, pk)
    assert got["length"] == [60001, 65530] and got["caplens"] == [34 + 60001, 34 + 65530]
    second = got["data"][got["offsets"][1]:]
    assert bytes(second[16:18]) == b"\x00\x00" and flowcases.csum(bytes(second[14:34])) == 0
