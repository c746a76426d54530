"""gpk_dns_batch on the device against the model (dns_model.py), byte for byte:
every verdict, class boundary, index, message record, entry record and name
byte, with the outputs pre-filled so that a stray write shows; the compaction
at wave and block boundaries; the capacity rules with the retry; the composed
DecodeBatch, one VXLAN level included. No tolerance anywhere. Messages stay at
or under 1500 bytes."""
import numpy as np
import pytest
import torch

import configs
import dns_model as M
import dnscases as C
import tunnelcases as TC
from dnsutil import GOLDEN, assert_same_dns, dns_parser, golden_packet, pcap_dns_frames
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition

pytestmark = pytest.mark.gpu
CASES, EXPECT = C.quirk_cases()
PACKETS = [p for _, p in CASES]
FILL32 = -1515870811  # 0xA5A5A5A5


def dev(a):
    a = np.array(a)  # a writable copy
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_dns(ctx, cfg, data, offs, caps, rr_cap, name_cap, dnd=None, stream=None):
    """Decode with layouts and run the DNS pass on the device; outputs start
    as 0xA5 bytes. Returns (outputs as host arrays, decode results as host arrays)."""
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
               rrs=torch.full((rr_cap * 96,), 0xA5, dtype=torch.uint8, device="cuda"),
               names=torch.full((name_cap,), 0xA5, dtype=torch.uint8, device="cuda"))
    own = dnd is None
    dnd = dnd or flows.DNSDecoder(max(n, 1))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    dnd.decode(ctx, d, o, c, rec, lay, p, rr_cap, name_cap, out=out, stream=stream)
    torch.cuda.synchronize()
    if own:
        dnd.close()
    h = dict(verdict=out["verdict"].cpu().numpy(), class_start=out["class_start"].cpu().numpy().view(np.uint32),
             index=out["index"].cpu().numpy().view(np.uint32), records=out["records"].cpu().numpy().view(_lib.DNS_DTYPE),
             counts=out["counts"].cpu().numpy().view(np.uint32), rrs=out["rrs"].cpu().numpy().view(_lib.DNS_RR_DTYPE),
             names=out["names"].cpu().numpy())
    r = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
             flows=fl.cpu().numpy().view(np.uint64), layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE))
    return h, r


def model_dns(cfg, data, offs, caps, rr_cap=None, name_cap=None):
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    return M.dns(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], rr_cap, name_cap, fill=0xA5), ref


def check(ctx, cfg, packets, align=1, pad=0, spare=(3, 5), **kw):
    """The device against the model on whole arrays; the arenas are `spare`
    entries and bytes longer than needed: the device must leave those at 0xA5."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    exact, _ = model_dns(cfg, data, offs, caps)
    rr_cap, name_cap = len(exact["rrs"]) + spare[0], len(exact["names"]) + spare[1]
    m, ref = model_dns(cfg, data, offs, caps, rr_cap, name_cap)
    h, r = device_dns(ctx, cfg, data, offs, caps, rr_cap, name_cap, **kw)
    configs.assert_same(r, ref, "decode")
    assert_same_dns(m, h, "device")  # whole arrays: what the model leaves at 0xA5 the device must not touch
    return m, h


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_cases_and_golden_packets(gpu_ctx, cfg):
    """Every case, the harvested vectors and the capture. The deepest walk is
    pointer_loop_255_levels: 255 levels of 126 labels, about 32 K steps in one
    lane before level 256 fails."""
    pk = PACKETS + [golden_packet(v)[0] for v in GOLDEN] + pcap_dns_frames() + list(C.layers17())
    m, h = check(gpu_ctx, cfg, pk)
    assert int(m["counts"][1]) > 40 and int(m["counts"][2]) > 40
    assert int(h["verdict"][-1]) == _lib.DNS_UNKNOWN
    assert np.all(h["records"][int(h["counts"][0]):].view(np.uint8) == 0xA5)  # nothing written past the list
    errs = {int(e) for e in h["records"][:int(h["counts"][0])]["err"]}
    assert errs >= set(M.ALL_ERRORS)


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_fuzz_corpus(gpu_ctx, fuzz, align, pad):
    check(gpu_ctx, C.PARSER, fuzz, align=align, pad=pad)


def class_samples():
    c = dict(CASES)
    # an OK and a failed message alternate, with different entry and name sizes; and a plain packet
    return [c["resp_soa"], c["qname_0x40"], c["query_a"], c["short_11"], c["resp_all_sections"], c["counts_zero"]], \
        c["plain_tcp"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_compaction_sizes(gpu_ctx, n):
    """Candidate counts around the wave (64) and the block (256), in all-candidate, no-candidate and
    alternating batches."""
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
    dnd = flows.DNSDecoder(600)
    for n in (600, 5, 300):
        pk = [cand[i % 6] if i % 3 else plain for i in range(n)]
        check(gpu_ctx, C.PARSER, pk, dnd=dnd)
    with pytest.raises(_lib.GpkError):
        data, offs, caps = pack([plain] * 601)
        device_dns(gpu_ctx, C.PARSER, data, offs, caps, 4, 4, dnd=dnd)
    dnd.close()


def test_stream_and_device_are_left_alone(gpu_ctx):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    before = torch.cuda.current_device()
    dnd = flows.DNSDecoder(len(PACKETS), before)
    check(gpu_ctx, C.PARSER, PACKETS, dnd=dnd, stream=torch.cuda.Stream())
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = flows.DNSDecoder(16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    dnd.close()
    assert torch.cuda.current_device() == before


def test_capacity_rules_and_retry(gpu_ctx):
    """Exact fit, one short in each arena, zero capacities, half: whole
    messages or nothing, nothing at or past a capacity; then decode_all's
    retry from capacities of 1."""
    pk = PACKETS[:24] * 3
    data, offs, caps = pack(pk)
    full, _ = model_dns(C.PARSER, data, offs, caps)
    need_rr, need_nb = len(full["rrs"]), len(full["names"])
    for rr_cap, name_cap in ((need_rr, need_nb), (need_rr - 1, need_nb), (need_rr, need_nb - 1), (0, need_nb),
                             (need_rr, 0), (0, 0), (need_rr // 2, need_nb // 2)):
        m, _ = model_dns(C.PARSER, data, offs, caps, rr_cap, name_cap)
        h, _ = device_dns(gpu_ctx, C.PARSER, data, offs, caps, rr_cap, name_cap)
        assert_same_dns(m, h, "caps %d %d" % (rr_cap, name_cap))
        assert int(h["counts"][3]) == int(rr_cap < need_rr or name_cap < need_nb)
        assert flows.DNSDecoder.needed(h["counts"]) == (need_rr, need_nb)
    p = configs.device_parser(C.PARSER)
    n = len(caps)
    d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
    o, c = dev(offs), dev(caps)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(p, d, o, c, rec, torch.zeros(2 * n, dtype=torch.int32, device="cuda"),
                          torch.zeros(3 * n, dtype=torch.int64, device="cuda"), lay)
    dnd = flows.DNSDecoder(n)
    out = dnd.decode_all(gpu_ctx, d, o, c, rec, lay, p, rr_cap=1, name_cap=1)
    torch.cuda.synchronize()
    dnd.close()
    assert not int(out["counts"][3].item())
    assert out["rrs"].cpu().numpy().tobytes() == full["rrs"].tobytes()
    assert out["names"].cpu().numpy().tobytes() == full["names"].tobytes()


def test_argument_faults(gpu_ctx):
    data, offs, caps = pack(PACKETS[:4])
    with pytest.raises(_lib.GpkError):  # data not 16-byte aligned
        n = len(caps)
        p = configs.device_parser(C.PARSER)
        d = dev(np.concatenate([np.zeros(1, np.uint8), data, np.zeros(32, np.uint8)]))[1:]
        dnd = flows.DNSDecoder(n)
        try:
            dnd.decode(gpu_ctx, d, dev(offs), dev(caps), torch.zeros(n * 16, dtype=torch.uint8, device="cuda"),
                       torch.zeros(n * 64, dtype=torch.uint8, device="cuda"), p, 4, 4)
        finally:
            dnd.close()
    with pytest.raises(_lib.GpkError):
        flows.DNSDecoder(0)
    with pytest.raises(_lib.GpkError):
        flows.DNSDecoder(1 << 28)


# ---- the composed DecodeBatch ---------------------------------------------------------------------
def real_parser(cfg=C.PARSER, ctx=None, **kw):
    p = dns_parser(cfg, **kw)
    p._host_decoder = None  # the device decodes
    p._ctx = ctx
    return p


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_decode_batch_composed(gpu_ctx, cfg, fuzz):
    pk = PACKETS + fuzz[:1000]
    want = M.compose(cfg, pk)
    res = real_parser(cfg, gpu_ctx).DecodeBatch(G.PacketBatch.from_packets(pk))
    assert isinstance(res, G.TunnelBatchResult) and len(res.levels) == 1
    check_composition(res, want, len(pk))
    got, exp = res.levels[0][0].dns, want["levels"][0][0]["dns"]
    m = int(exp["counts"][0])
    assert np.array_equal(got["verdict"], exp["verdict"]) and got["records"].tobytes() == exp["records"][:m].tobytes()
    assert got["rrs"].tobytes() == exp["rrs"].tobytes() and got["names"].tobytes() == exp["names"].tobytes()


def test_capture_on_the_device_with_and_without_the_layer(gpu_ctx):
    frames = pcap_dns_frames()
    p = real_parser(ctx=gpu_ctx)
    res = p.DecodeBatch(G.PacketBatch.from_packets(frames))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == [17, 20, 45, 107]
    assert [(q.Name, int(q.Type)) for q in p._dns.Questions] == [(b"picslife.ru", 1)] and p._dns.ID == 63000
    assert all([int(t) for t in res.Decoded(i)] == [17, 20, 45, 107] and res.Err(i) is None for i in range(len(frames)))
    q = real_parser(ctx=gpu_ctx, extra=())
    plain = q.DecodeBatch(G.PacketBatch.from_packets(frames), layouts=True)
    assert not isinstance(plain, G.TunnelBatchResult)
    assert [int(t) for t in plain.Decoded(0)] == [17, 20, 45] and plain.Err(0).Error() == "No decoder for layer type DNS"
    with pytest.raises(ValueError, match="fields=True"):
        p.DecodeBatch(G.PacketBatch.from_packets(frames), fields=True)


def test_decode_batch_with_a_vxlan_level(gpu_ctx):
    c = dict(CASES)
    pk = [TC.over_udp(TC.vxlan(c["resp_soa"]), TC.VX), c["query_a"], TC.over_udp(TC.vxlan(TC.inner_eth()), TC.VX),
          TC.over_udp(TC.vxlan(c["qname_0x40"]), TC.VX), c["plain_tcp"], TC.over_udp(TC.vxlan(c["short_11"]), TC.VX)] * 9
    want = M.compose(C.PARSER, pk, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 20, 45, 107]
    p = real_parser(C.PARSER, gpu_ctx, tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._dns.Answers[0].SOA.RName == b"admin.example.com" and p._tunnels[2].VNI == 0x123456
