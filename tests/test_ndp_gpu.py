"""gpk_ndp_batch on the device against the model (ndp_model.py), byte for byte:
every verdict, class boundary, index, message record and entry descriptor, with
the outputs pre-filled with 0xA5 so that a stray write shows; the compaction at
wave and block boundaries; the capacity rule with the retry; the composed
DecodeBatch, one VXLAN level included. No tolerance anywhere."""
import numpy as np
import pytest
import torch

import configs
import controlcases as CC
import ndp_model as M
import ndpcases as C
import tunnelcases as TC
from ndputil import (CASES, CONTROLS, GOLDEN_PACKETS, NAMES, PACKETS, assert_same_ndp, corpus, device_arrays,
                     ndp_parser)
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition

pytestmark = pytest.mark.gpu
FILL32 = -1515870811  # 0xA5A5A5A5
ALL_ERRORS = set(range(_lib.NDP_ERR_FIRST, _lib.NDP_ERR_END))


def dev(a):
    a = np.array(a)  # a writable copy
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_ndp(ctx, cfg, data, offs, caps, entry_cap, kinds=M.ALL, ndd=None, stream=None):
    """Decode with layouts and run the NDP pass on the device; outputs start as
    0xA5 bytes. Returns (outputs as host arrays, decode results as host arrays)."""
    n = len(caps)
    p = configs.device_parser(cfg)
    d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
    o, c = dev(offs), dev(caps)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    ctx.decode_device(p, d, o, c, rec, err, fl, lay)
    out = dict(verdict=torch.full((n,), FILL32, dtype=torch.int32, device="cuda"),
               class_start=torch.full((3,), FILL32, dtype=torch.int32, device="cuda"),
               index=torch.full((n,), FILL32, dtype=torch.int32, device="cuda"),
               records=torch.full((n * 64,), 0xA5, dtype=torch.uint8, device="cuda"),
               counts=torch.full((8,), FILL32, dtype=torch.int32, device="cuda"),
               entries=torch.full((entry_cap * 16,), 0xA5, dtype=torch.uint8, device="cuda"))
    own = ndd is None
    ndd = ndd or flows.NDPDecoder(max(n, 1))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    ndd.decode(ctx, d, o, c, rec, lay, p, entry_cap, kinds, out=out, stream=stream)
    torch.cuda.synchronize()
    if own:
        ndd.close()
    r = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
             flows=fl.cpu().numpy().view(np.uint64), layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE))
    return device_arrays(out), r


def model_ndp(cfg, data, offs, caps, entry_cap=None, kinds=M.ALL):
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    args = (cfg, data, offs, caps, ref["records"], ref["layouts"], kinds)
    if entry_cap is None:
        entry_cap = flows.NDPDecoder.needed(M.ndp(*args, entry_cap=0)["counts"])
    return M.ndp(*args, entry_cap=entry_cap, fill=0xA5), ref


def check(ctx, cfg, packets, align=1, pad=0, spare=3, kinds=M.ALL, **kw):
    """The device against the model on whole arrays; the arena is `spare`
    entries longer than needed: the device must leave those at 0xA5."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    exact, _ = model_ndp(cfg, data, offs, caps, kinds=kinds)
    cap = len(exact["entries"]) + spare
    m, ref = model_ndp(cfg, data, offs, caps, cap, kinds)
    h, r = device_ndp(ctx, cfg, data, offs, caps, cap, kinds, **kw)
    configs.assert_same(r, ref, "decode")
    assert_same_ndp(m, h, "device")  # whole arrays: what the model leaves at 0xA5 the device must not touch
    return m, h


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_cases_and_golden_packets(gpu_ctx, cfg):
    pk = PACKETS + GOLDEN_PACKETS + list(C.layers17())
    m, h = check(gpu_ctx, cfg, pk)
    assert int(m["counts"][1]) > 40 and int(m["counts"][2]) > 25
    assert int(h["verdict"][-1]) == _lib.NDP_UNKNOWN and int(h["verdict"][-2]) >= 0
    assert np.all(h["records"][int(h["counts"][0]):].view(np.uint8) == 0xA5)  # nothing written past the list
    assert {int(e) for e in h["records"][:int(h["counts"][0])]["err"]} - {0} == ALL_ERRORS


def test_kinds_on_the_device(gpu_ctx):
    """A parser without layers.ICMPv6 (way 2 only), and single kinds."""
    for kinds in (M.ALL & ~M.ICMP6, M.ICMP6 | 4, M.ALL & ~4):
        check(gpu_ctx, C.PARSER, PACKETS, kinds=kinds)


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_corpus(gpu_ctx, align, pad):
    check(gpu_ctx, C.PARSER, corpus(), align=align, pad=pad)


def class_samples():
    c = dict(CASES)
    # decoded and failed messages alternate, with 3, 0, 2, 0, 1 and 0 entries; and a plain packet
    return [c["ra_three_options"], c["option_length_0"], c["mld2_report_2_records"], c["mld2_report_aux_overruns"],
            c["ns_one_option"], c["mld_query_24_is_v2"]], c["plain_udp"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_compaction_sizes(gpu_ctx, n):
    """Candidate counts around the wave (64) and the block (256), in
    all-candidate, no-candidate and alternating batches."""
    cand, plain = class_samples()
    for pattern in ("all", "none", "alternating"):
        pk = [plain if pattern == "none" or (pattern == "alternating" and i & 1) else
              cand[(i // 2 if pattern == "alternating" else i) % 6] for i in range(n)]
        m, h = check(gpu_ctx, C.PARSER, pk)
        want = 0 if pattern == "none" else n if pattern == "all" else (n + 1) // 2
        assert int(h["counts"][0]) == want
        if pattern != "none" and n >= 64:
            assert all(int(x) > 0 for x in h["counts"][1:3])
        for c in range(2):  # ordered by class, then by packet index
            idx = h["index"][int(h["class_start"][c]):int(h["class_start"][c + 1])]
            assert np.all(np.diff(idx.astype(np.int64)) > 0)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257])
def test_candidate_count_among_plain_packets(gpu_ctx, m):
    """Exactly m candidates scattered over 1500 packets (six blocks)."""
    cand, plain = class_samples()
    rnd = np.random.RandomState(m)
    where = set(rnd.choice(1500, m, replace=False).tolist())
    pk = [cand[i % 6] if i in where else plain for i in range(1500)]
    _, h = check(gpu_ctx, C.PARSER, pk)
    assert int(h["counts"][0]) == m


def test_candidates_only_in_the_last_block(gpu_ctx):
    cand, plain = class_samples()
    pk = [plain] * 1024 + [cand[i % 6] for i in range(37)]
    _, h = check(gpu_ctx, C.PARSER, pk)
    assert int(h["counts"][0]) == 37 and int(h["index"].view(np.uint32)[:37].min()) == 1024


def test_one_decoder_serves_batches_of_different_sizes(gpu_ctx):
    cand, plain = class_samples()
    ndd = flows.NDPDecoder(600)
    for n in (600, 5, 300):
        pk = [cand[i % 6] if i % 3 else plain for i in range(n)]
        check(gpu_ctx, C.PARSER, pk, ndd=ndd)
    with pytest.raises(_lib.GpkError):
        data, offs, caps = pack([plain] * 601)
        device_ndp(gpu_ctx, C.PARSER, data, offs, caps, 4, ndd=ndd)
    ndd.close()


def test_stream_and_device_are_left_alone(gpu_ctx):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    before = torch.cuda.current_device()
    ndd = flows.NDPDecoder(len(PACKETS), before)
    check(gpu_ctx, C.PARSER, PACKETS, ndd=ndd, stream=torch.cuda.Stream())
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = flows.NDPDecoder(16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    ndd.close()
    assert torch.cuda.current_device() == before


def test_capacity_rule_and_retry(gpu_ctx):
    """Exact fit, one entry short, capacity 0, half: whole messages or nothing,
    nothing at or past the capacity; then decode_all's retry from capacities of
    0 and 1."""
    pk = PACKETS * 3
    data, offs, caps = pack(pk)
    full, _ = model_ndp(C.PARSER, data, offs, caps)
    need = len(full["entries"])
    assert need > 60
    for cap in (need, need - 1, 0, 1, need // 2):
        m, _ = model_ndp(C.PARSER, data, offs, caps, cap)
        h, _ = device_ndp(gpu_ctx, C.PARSER, data, offs, caps, cap)
        assert_same_ndp(m, h, "cap %d" % cap)
        assert int(h["counts"][3]) == int(cap < need) and flows.NDPDecoder.needed(h["counts"]) == need
    p = configs.device_parser(C.PARSER)
    n = len(caps)
    d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
    o, c = dev(offs), dev(caps)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(p, d, o, c, rec, torch.zeros(2 * n, dtype=torch.int32, device="cuda"),
                          torch.zeros(3 * n, dtype=torch.int64, device="cuda"), lay)
    ndd = flows.NDPDecoder(n)
    for first in (0, 1):
        out = ndd.decode_all(gpu_ctx, d, o, c, rec, lay, p, entry_cap=first)
        torch.cuda.synchronize()
        assert not int(out["counts"][3].item())
        assert out["entries"].cpu().numpy().tobytes() == full["entries"].tobytes()
        m = int(full["counts"][0])
        assert out["records"].cpu().numpy()[:m * 64].tobytes() == full["records"][:m].tobytes()
    ndd.close()


def test_argument_faults(gpu_ctx):
    data, offs, caps = pack(PACKETS[:4])
    n = len(caps)
    p = configs.device_parser(C.PARSER)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    ndd = flows.NDPDecoder(n)
    try:
        with pytest.raises(_lib.GpkError):  # data not 16-byte aligned
            d = dev(np.concatenate([np.zeros(1, np.uint8), data, np.zeros(32, np.uint8)]))[1:]
            ndd.decode(gpu_ctx, d, dev(offs), dev(caps), rec, lay, p, 4)
        d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
        for kinds in (0, _lib.NDP_ICMP6, 4096):
            with pytest.raises(_lib.GpkError):
                ndd.decode(gpu_ctx, d, dev(offs), dev(caps), rec, lay, p, 4, kinds)
    finally:
        ndd.close()
    with pytest.raises(_lib.GpkError):
        flows.NDPDecoder(0)
    with pytest.raises(_lib.GpkError):
        flows.NDPDecoder(1 << 28)


# ---- the composed DecodeBatch ---------------------------------------------------------------------
def real_parser(cfg=C.PARSER, ctx=None, **kw):
    p = ndp_parser(cfg, **kw)
    p._host_decoder = None  # the device decodes
    p._ctx = ctx
    return p


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_decode_batch_composed(gpu_ctx, cfg):
    pk = PACKETS + GOLDEN_PACKETS + corpus()[:1000]
    want = M.compose(cfg, pk)
    p = real_parser(cfg, gpu_ctx)
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    assert isinstance(res, G.TunnelBatchResult) and len(res.levels) == 1
    check_composition(res, want, len(pk))
    got, exp = res.levels[0][0].ndp, want["levels"][0][0]["ndp"]
    m = int(exp["counts"][0])
    assert np.array_equal(got["verdict"], exp["verdict"]) and got["records"].tobytes() == exp["records"][:m].tobytes()
    assert got["entries"].tobytes() == exp["entries"].tobytes()
    decoded = []
    i = NAMES.index("ra_three_options")
    assert res.Hydrate(i, decoded) is None and [int(t) for t in decoded] == [17, 21, 57, 125]
    assert [int(o.Type) for o in p._ndps[_lib.NDP_RA].Options] == [1, 5, 3] and len(res.NDP(i)[1]) == 3
    with pytest.raises(ValueError, match="fields=True"):
        p.DecodeBatch(G.PacketBatch.from_packets(pk[:4]), fields=True)


def test_decode_batch_without_the_layers_is_the_control_pass(gpu_ctx):
    """A parser that holds the control layers only runs what it ran before."""
    import control_model as CM
    pk = PACKETS + corpus()[:256]
    want = CM.compose(C.PARSER, pk)
    res = real_parser(C.PARSER, gpu_ctx, extra=CONTROLS).DecodeBatch(G.PacketBatch.from_packets(pk))
    check_composition(res, want, len(pk))
    assert all(part.ndp is None for lvl in res.levels for part in lvl)
    i = NAMES.index("ns_one_option")
    assert res.Err(i).Error() == "No decoder for layer type ICMPv6NeighborSolicitation"


def test_decode_batch_with_a_vxlan_level(gpu_ctx):
    c, cc = dict(CASES), dict(CC.quirk_cases()[0])
    pk = [TC.over_udp(TC.vxlan(c["ra_three_options"]), TC.VX), c["ns_one_option"], TC.over_udp(TC.vxlan(TC.inner_eth()), TC.VX),
          TC.over_udp(TC.vxlan(c["option_length_0"]), TC.VX), c["plain_udp"], cc["icmp6_echo_request"],
          TC.over_udp(TC.vxlan(c["mld2_report_2_records"]), TC.VX), TC.over_udp(TC.vxlan(cc["arp_request_42"]), TC.VX)] * 9
    want = M.compose(C.PARSER, pk, control_kinds=15, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 21, 57, 125]
    p = real_parser(C.PARSER, gpu_ctx, tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(6, decoded) is None and [int(t) for t in decoded] == want["decoded"][6]
    assert len(p._ndps[_lib.NDP_MLD2_REPORT].MulticastAddressRecords) == 2 and p._tunnels[2].VNI == 0x123456
