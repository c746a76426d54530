"""gpk_tunnel_batch on the device against the model (tunnel_model.py), bit for
bit: every verdict, class boundary, index, offset, length and record byte; the
compaction at block and wave boundaries; the GRE sum at every alignment and on
both sides of the lane-group threshold; the composed DecodeBatch; table edits.
No tolerance anywhere."""
import numpy as np
import pytest
import torch

import configs
import tunnel_model as M
import tunnelcases as C
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import GOLDEN, assert_same_peel, check_composition, golden_packet, tunnel_parser

pytestmark = pytest.mark.gpu
CASES, _ = C.quirk_cases()


def dev(a):
    a = np.array(a)  # a writable copy
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_peel(ctx, cfg, data, offs, caps, kinds=7, gre_checksum=True, threshold=None, det=None):
    """Decode with layouts and peel on the device; outputs start as 0xA5 bytes.
    Returns (peel outputs as host arrays, decode results as host arrays)."""
    n = len(caps)
    p = configs.device_parser(cfg)
    d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
    o, c = dev(offs), dev(caps)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    ctx.decode_device(p, d, o, c, rec, err, fl, lay)
    out = dict(verdict=torch.full((n,), -1515870811, dtype=torch.int32, device="cuda"),
               class_start=torch.full((7,), -1515870811, dtype=torch.int32, device="cuda"),
               index=torch.full((n,), -1515870811, dtype=torch.int32, device="cuda"),
               in_offsets=torch.full((n,), -6510615555426900571, dtype=torch.int64, device="cuda"),
               in_caplens=torch.full((n,), -1515870811, dtype=torch.int32, device="cuda"),
               tunnels=torch.full((n * 72,), 0xA5, dtype=torch.uint8, device="cuda"),
               counts=torch.full((8,), -1515870811, dtype=torch.int32, device="cuda"))
    own = det is None
    det = det or flows.Detunneler(max(n, 1))
    if threshold is not None:
        det.set_sum_threshold(threshold)
    det.peel(ctx, d, o, c, rec, lay, p, kinds, gre_checksum, out=out)
    torch.cuda.synchronize()
    if own:
        det.close()
    h = dict(verdict=out["verdict"].cpu().numpy(), class_start=out["class_start"].cpu().numpy().view(np.uint32),
             index=out["index"].cpu().numpy().view(np.uint32), in_offsets=out["in_offsets"].cpu().numpy().view(np.uint64),
             in_caplens=out["in_caplens"].cpu().numpy().view(np.uint32),
             tunnels=out["tunnels"].cpu().numpy().view(_lib.TUNNEL_DTYPE), counts=out["counts"].cpu().numpy().view(np.uint32))
    r = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
             flows=fl.cpu().numpy().view(np.uint64), layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE))
    return h, r


def model_peel(cfg, data, offs, caps, kinds=7, gre_checksum=True):
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    return M.peel(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], kinds, gre_checksum, fill=0xA5), ref


def check(ctx, cfg, packets, align=1, pad=0, **kw):
    data, offs, caps = pack(packets, align=align, pad=pad)
    m, ref = model_peel(cfg, data, offs, caps, kw.get("kinds", 7), kw.get("gre_checksum", True))
    h, r = device_peel(ctx, cfg, data, offs, caps, **kw)
    configs.assert_same(r, ref, "outer decode")
    assert_same_peel(m, h, "device")  # whole arrays: what the model leaves at 0xA5 the device must not touch
    return m, h


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_golden_and_quirk_packets(gpu_ctx, cfg):
    pk = [p for _, p in CASES] + [golden_packet(v)[1] for v in GOLDEN if not v.get("skip")]
    m, _ = check(gpu_ctx, cfg, pk)
    assert int(m["counts"][0]) > 50 and all(int(x) for x in m["counts"][1:8])


def test_golden_behind_linux_sll(gpu_ctx):
    cfg, pkt, _ = golden_packet([v for v in GOLDEN if v["name"] == "TestDecodeGeneve1"][0])
    m, _ = check(gpu_ctx, cfg, [pkt])
    assert int(m["counts"][0]) == 1


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_fuzz_corpus(gpu_ctx, fuzz, align, pad):
    check(gpu_ctx, C.PARSER, fuzz, align=align, pad=pad)


@pytest.mark.parametrize("kinds,csum", [(1, True), (2, True), (4, False), (7, False)])
def test_kinds_and_flags(gpu_ctx, fuzz, kinds, csum):
    check(gpu_ctx, C.PARSER, fuzz[:700], kinds=kinds, gre_checksum=csum)


def class_samples():
    c = dict(CASES)
    # one packet per class, in an order that interleaves them, and a plain one
    return [c["gre_plain"], c["vxlan_plain"], c["geneve_len6"], c["geneve_dot1q"], c["gre_ipv6"], c["geneve_unregistered"]], \
        c["plain_tcp"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 1025])
def test_compaction_sizes(gpu_ctx, n):
    cand, plain = class_samples()
    for pattern in ("all", "none", "alternating"):
        pk = [plain if pattern == "none" or (pattern == "alternating" and i & 1) else cand[(i // 2 if pattern == "alternating"
                                                                                           else i) % 6] for i in range(n)]
        m, h = check(gpu_ctx, C.PARSER, pk)
        want = 0 if pattern == "none" else n if pattern == "all" else (n + 1) // 2
        assert int(h["counts"][0]) == want
        if pattern != "none" and n >= 64:
            assert all(int(x) > 0 for x in h["counts"][1:7])  # the classes interleave inside every wave
        # ordered by class, then by packet index
        for c in range(6):
            idx = h["index"][int(h["class_start"][c]):int(h["class_start"][c + 1])]
            assert np.all(np.diff(idx.astype(np.int64)) > 0)


def test_one_tunneler_serves_batches_of_different_sizes(gpu_ctx):
    cand, plain = class_samples()
    det = flows.Detunneler(600)
    for n in (600, 5, 300):
        pk = [cand[i % 6] if i % 3 else plain for i in range(n)]
        data, offs, caps = pack(pk)
        m, _ = model_peel(C.PARSER, data, offs, caps)
        h, _ = device_peel(gpu_ctx, C.PARSER, data, offs, caps, det=det)
        assert_same_peel(m, h)
    with pytest.raises(_lib.GpkError):
        data, offs, caps = pack([plain] * 601)
        device_peel(gpu_ctx, C.PARSER, data, offs, caps, det=det)
    det.close()


# ---- the GRE sum ------------------------------------------------------------------------------
GRE_DIRECT = dict(C.PARSER, ethertype={0x9998: 18})  # Ethernet -> GRE: no length field limits the slice


def gre_sum_batch(lengths, good=True, cbit=True):
    """Ethernet / GRE packets whose GRE slice has each length in `lengths`, at
    every start alignment mod 16: (data, offsets, caplens)."""
    rnd = np.random.RandomState(7)
    pk, offs, pos = [], [], 0
    for ln in lengths:
        for a in range(16):
            body = bytes(rnd.randint(0, 256, max(ln - 8, 0), dtype=np.uint8))
            g = C.gre_with_checksum(body, 0x0800, good=good) if cbit else C.gre(body + bytes(4), 0x0800)
            p = C.eth(g[:ln], 0x9998)
            pos = (pos + 15) // 16 * 16 + (a - 14) % 16  # the GRE header starts at alignment a
            offs.append(pos)
            pk.append(p)
            pos += len(p)
    data = np.zeros(pos + 64, np.uint8)
    for o, p in zip(offs, pk):
        data[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return data, np.array(offs, np.uint64), np.array([len(p) for p in pk], np.uint32)


@pytest.mark.parametrize("threshold", [None, 24, 1])
def test_gre_sum_lengths_and_alignments(gpu_ctx, threshold):
    """Slices of 4..40 bytes and on both sides of the lane-group threshold
    (GPK_TUN_SUM_GROUP_BYTES), at every start alignment; with the threshold
    lowered the short slices take the 64-lane kernel too."""
    T = _lib.TUN_SUM_GROUP_BYTES
    lengths = list(range(4, 41)) + [1791, 1792, 1793, T - 2, T - 1, T, T + 1, T + 2, T + 15, T + 16, T + 1023, T + 1024, T + 1025]
    for good in (True, False):
        data, offs, caps = gre_sum_batch(lengths, good=good)
        m, _ = model_peel(GRE_DIRECT, data, offs, caps)
        h, _ = device_peel(gpu_ctx, GRE_DIRECT, data, offs, caps, threshold=threshold)
        assert_same_peel(m, h, "gre sum")
        n = int(h["counts"][0])
        assert n == len(caps) and int(h["counts"][7]) == 16 * len([x for x in lengths if x >= 8])
        st = h["tunnels"][:n]["status"]
        ok = h["tunnels"][:n]["err"] == 0
        # whole slices verify; a slice cut short of its checksummed bytes almost never does
        assert np.all((st[ok] & 2) == 2) and (np.all(st[ok] & 4) if good else not np.any(st[ok] & 4))


def test_gre_sum_c_clear(gpu_ctx):
    data, offs, caps = gre_sum_batch([8, 9, 40, 1800], cbit=False)
    m, _ = model_peel(GRE_DIRECT, data, offs, caps)
    h, _ = device_peel(gpu_ctx, GRE_DIRECT, data, offs, caps)
    assert_same_peel(m, h)
    assert int(h["counts"][7]) == 0 and np.all(h["tunnels"][:len(caps)]["status"] == 4)


@pytest.mark.parametrize("size", [70000, 140001])
def test_gre_sum_mod_2_32(gpu_ctx, size):
    """One saturated slice: 70 000 bytes of 0xFF sum past 2^31, 140 001 wrap 2^32
    (ComputeChecksum wraps before the single fold)."""
    g = bytearray(C.gre(b"\xff" * (size - 8), 0x0800, b0=0x80, csum=0xBEEF, off=0xFFFF))
    pk = [C.eth(bytes(g), 0x9998), dict(CASES)["gre_checksum_good"]]
    data, offs, caps = pack(pk, pad=5)
    m, _ = model_peel(GRE_DIRECT, data, offs, caps)
    h, _ = device_peel(gpu_ctx, GRE_DIRECT, data, offs, caps)
    assert_same_peel(m, h)
    total = sum(g[i] << 8 | g[i + 1] for i in range(0, size - 1, 2)) + ((g[-1] << 8) if size & 1 else 0)
    assert (total >= 1 << 32) == (size > 140000) and total >= 1 << 31
    assert int(h["tunnels"][int(h["verdict"][0])]["gre_correct"]) == M.fold((total - 0xBEEF) & 0xffffffff)


# ---- the composed DecodeBatch ---------------------------------------------------------------------
def real_parser(cfg=C.PARSER, ctx=None, tunnels=(L.GRE, L.VXLAN, L.Geneve)):
    p = tunnel_parser(cfg, tunnels)
    p._host_decoder = None  # the device decodes
    p._ctx = ctx
    return p


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_decode_batch_composed(gpu_ctx, cfg, fuzz):
    """VXLAN/IPv4/TCP, Geneve/IPv6/UDP with options, GRE/IPv4, GRE/0x6558, VXLAN
    inside GRE and Geneve in Geneve, mixed with plain packets and the fuzz
    corpus: decoded, error text, Truncated, and each level's records, flows and
    checksums against model + oracle."""
    pk = [p for _, p in CASES] + fuzz[:1000]
    want = M.compose(cfg, pk)
    res = real_parser(cfg, gpu_ctx).DecodeBatch(G.PacketBatch.from_packets(pk))
    assert isinstance(res, G.TunnelBatchResult) and len(res.levels) >= 3
    check_composition(res, want, len(pk))


def test_decode_layers_and_hydrate_on_device(gpu_ctx):
    p = real_parser(ctx=gpu_ctx)
    c = dict(CASES)
    decoded = []
    assert p.DecodeLayers(c["vxlan_in_gre"], decoded) is None
    assert [int(t) for t in decoded] == [17, 20, 18, 20, 45, 116, 17, 20, 44, 2]
    assert p._tunnels[2].VNI == 0x123456 and p._tunnels[1].Protocol == 0x0800
    res = p.DecodeBatch(G.PacketBatch.from_packets([c["gre_checksum_bad"], c["gre_over_ip6_geneve_ip6_udp"]]))
    assert res.Hydrate(0, decoded) is None
    _, r = p._tunnels[1].VerifyChecksum()
    assert not r.Valid and r.Actual == r.Correct ^ 0x0100
    err = res.Hydrate(1, decoded)
    assert err.Error() == "No decoder for layer type DNS" and [o.Length for o in p._tunnels[4].Options] == [12]
    lvl2 = res.Level(2)[0]
    assert int(lvl2.first) == 17 and list(lvl2.index) == [1] and lvl2.result.FlowHashes(0)[2] is not None


def test_parser_without_tunnel_layers_is_byte_identical(gpu_ctx, fuzz):
    pk = fuzz[:500]
    b = G.PacketBatch.from_packets(pk)
    res = real_parser(ctx=gpu_ctx, tunnels=()).DecodeBatch(b, layouts=True)
    assert isinstance(res, G.BatchResult)
    n = len(pk)
    d, o, c = dev(b.data), dev(b.offsets), dev(b.caplens)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(configs.device_parser(C.PARSER), d, o, c, rec, err, fl, lay)
    torch.cuda.synchronize()
    assert res.records.tobytes() == rec.cpu().numpy().tobytes()
    assert res.flows.tobytes() == fl.cpu().numpy().tobytes()
    assert res.layouts.tobytes() == lay.cpu().numpy().tobytes()


def test_table_edits_reach_the_kernel(gpu_ctx):
    cfg = dict(C.PARSER, udp_port={8472: 116}, ethertype={0x9999: 20})
    ie = C.inner_eth()
    pk = [C.over_udp(C.vxlan(ie), 8472), C.over_ip(C.gre(ie[14:], 0x9999)), C.over_udp(C.vxlan(ie), 8473)] * 3
    m, h = check(gpu_ctx, cfg, pk)
    assert list(h["verdict"][:3]) == [0, 3, _lib.TUN_NONE] and list(h["class_start"]) == [0, 3, 3, 6, 6, 6, 6]
    _, h0 = check(gpu_ctx, C.PARSER, pk)
    assert int(h0["verdict"][0]) == _lib.TUN_NONE and int(h0["counts"][0]) == 3
