"""gpk_control_batch on the device against the model (control_model.py), record
byte for record byte: every verdict, class boundary, index and record; the
compaction at wave and block boundaries; the ICMPv4 / ICMPv6 sums at every
alignment, on both sides of the lane-group threshold and past 2^32; the
composed DecodeBatch, one VXLAN level included. No tolerance anywhere."""
import numpy as np
import pytest
import torch

import configs
import control_model as M
import controlcases as C
import tunnelcases as TC
from controlutil import GOLDEN, assert_same_control, control_parser
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition

pytestmark = pytest.mark.gpu
CASES, _ = C.quirk_cases()
PACKETS = [p for _, p in CASES]
FILL32 = -1515870811  # 0xA5A5A5A5


def dev(a):
    a = np.array(a)  # a writable copy
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_control(ctx, cfg, data, offs, caps, kinds=15, checksum=True, threshold=None, ctd=None, stream=None):
    """Decode with layouts and run the control pass on the device; outputs start
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
               class_start=torch.full((5,), FILL32, dtype=torch.int32, device="cuda"),
               index=torch.full((n,), FILL32, dtype=torch.int32, device="cuda"),
               records=torch.full((n * 64,), 0xA5, dtype=torch.uint8, device="cuda"),
               counts=torch.full((8,), FILL32, dtype=torch.int32, device="cuda"))
    own = ctd is None
    ctd = ctd or flows.ControlDecoder(max(n, 1))
    if threshold is not None:
        ctd.set_sum_threshold(threshold)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    ctd.decode(ctx, d, o, c, rec, lay, p, kinds, checksum, out=out, stream=stream)
    torch.cuda.synchronize()
    if own:
        ctd.close()
    h = dict(verdict=out["verdict"].cpu().numpy(), class_start=out["class_start"].cpu().numpy().view(np.uint32),
             index=out["index"].cpu().numpy().view(np.uint32),
             records=out["records"].cpu().numpy().view(_lib.CONTROL_DTYPE),
             counts=out["counts"].cpu().numpy().view(np.uint32))
    r = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
             flows=fl.cpu().numpy().view(np.uint64), layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE))
    return h, r


def model_control(cfg, data, offs, caps, kinds=15, checksum=True):
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    return M.control(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], kinds, checksum,
                     fill=0xA5), ref


def check(ctx, cfg, packets, align=1, pad=0, **kw):
    data, offs, caps = pack(packets, align=align, pad=pad)
    m, ref = model_control(cfg, data, offs, caps, kw.get("kinds", 15), kw.get("checksum", True))
    h, r = device_control(ctx, cfg, data, offs, caps, **kw)
    configs.assert_same(r, ref, "decode")
    assert_same_control(m, h, "device")  # whole arrays: what the model leaves at 0xA5 the device must not touch
    return m, h


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_golden_and_quirk_packets(gpu_ctx, cfg):
    pk = PACKETS + [bytes.fromhex(v["hex"]) for v in GOLDEN] + list(C.layers17())
    m, h = check(gpu_ctx, cfg, pk)
    assert int(m["counts"][0]) > 40 and all(int(x) for x in m["counts"][1:6])
    assert int(h["verdict"][-1]) == _lib.CTL_UNKNOWN
    assert np.all(h["records"][int(h["counts"][0]):].view(np.uint8) == 0xA5)  # nothing written past the list


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_fuzz_corpus(gpu_ctx, fuzz, align, pad):
    check(gpu_ctx, C.PARSER, fuzz, align=align, pad=pad)


@pytest.mark.parametrize("kinds,csum", [(1, True), (2, True), (4, False), (8, True), (11, False), (15, False)])
def test_kinds_and_flags(gpu_ctx, fuzz, kinds, csum):
    check(gpu_ctx, C.PARSER, fuzz[:700], kinds=kinds, checksum=csum)


def class_samples():
    c = dict(CASES)
    # one packet per class, in an order that interleaves them, and a plain one
    return [c["icmp6_echo_request"], c["arp_len7"], c["icmp4_echo"], c["arp_reply_padded_60"]], c["plain_tcp"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_compaction_sizes(gpu_ctx, n):
    """Candidate counts around the wave (64) and the scatter block (256), in all-candidate, no-candidate and
    alternating batches."""
    cand, plain = class_samples()
    for pattern in ("all", "none", "alternating"):
        pk = [plain if pattern == "none" or (pattern == "alternating" and i & 1) else
              cand[(i // 2 if pattern == "alternating" else i) % 4] for i in range(n)]
        m, h = check(gpu_ctx, C.PARSER, pk)
        want = 0 if pattern == "none" else n if pattern == "all" else (n + 1) // 2
        assert int(h["counts"][0]) == want
        if pattern != "none" and n >= 64:
            assert all(int(x) > 0 for x in h["counts"][1:5])
        for c in range(4):  # ordered by class, then by packet index
            idx = h["index"][int(h["class_start"][c]):int(h["class_start"][c + 1])]
            assert np.all(np.diff(idx.astype(np.int64)) > 0)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257])
def test_candidate_count_among_plain_packets(gpu_ctx, m):
    """Exactly m candidates scattered over 1500 packets (six blocks)."""
    cand, plain = class_samples()
    rnd = np.random.RandomState(m)
    where = set(rnd.choice(1500, m, replace=False).tolist())
    pk = [cand[i % 4] if i in where else plain for i in range(1500)]
    _, h = check(gpu_ctx, C.PARSER, pk)
    assert int(h["counts"][0]) == m


def test_candidates_only_in_the_last_block(gpu_ctx):
    cand, plain = class_samples()
    pk = [plain] * 1024 + [cand[i % 4] for i in range(37)]
    _, h = check(gpu_ctx, C.PARSER, pk)
    assert int(h["counts"][0]) == 37 and int(h["index"].view(np.uint32)[:37].min()) == 1024


def test_one_decoder_serves_batches_of_different_sizes(gpu_ctx):
    cand, plain = class_samples()
    ctd = flows.ControlDecoder(600)
    for n in (600, 5, 300):
        pk = [cand[i % 4] if i % 3 else plain for i in range(n)]
        data, offs, caps = pack(pk)
        m, _ = model_control(C.PARSER, data, offs, caps)
        h, _ = device_control(gpu_ctx, C.PARSER, data, offs, caps, ctd=ctd)
        assert_same_control(m, h)
    with pytest.raises(_lib.GpkError):
        data, offs, caps = pack([plain] * 601)
        device_control(gpu_ctx, C.PARSER, data, offs, caps, ctd=ctd)
    ctd.close()


def test_stream_and_device_are_left_alone(gpu_ctx):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    data, offs, caps = pack(PACKETS)
    m, _ = model_control(C.PARSER, data, offs, caps)
    before = torch.cuda.current_device()
    ctd = flows.ControlDecoder(len(caps), before)
    h, _ = device_control(gpu_ctx, C.PARSER, data, offs, caps, ctd=ctd, stream=torch.cuda.Stream())
    assert torch.cuda.current_device() == before
    assert_same_control(m, h)
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = flows.ControlDecoder(16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    ctd.close()
    assert torch.cuda.current_device() == before


# ---- the sums ----------------------------------------------------------------------------------
def sum_batch(lengths, v6, good=True):
    """Messages of each length in `lengths` at every start alignment mod 16:
    Ethernet / ICMPv4 through the private EtherType (no length field limits the
    slice), or Ethernet / IPv6 / ICMPv6. Returns (data, offsets, caplens)."""
    rnd = np.random.RandomState(11)
    pk, offs, pos = [], [], 0
    for ln in lengths:
        for a in range(16):
            if v6:
                body = bytes(rnd.randint(0, 256, max(ln - 4, 0), dtype=np.uint8))
                p = C.eth(C.ip6(C.icmp6(body, rnd.choice([1, 3, 128, 135]), good=good)[:ln], 58), 0x86dd)
                hdr = 54
            else:
                body = bytes(rnd.randint(0, 256, max(ln - 8, 0), dtype=np.uint8))
                p = C.eth(C.icmp4(body, good=good)[:ln], C.ET_ICMP4)
                hdr = 14
            pos = (pos + 15) // 16 * 16 + (a - hdr) % 16  # the message starts at alignment a
            offs.append(pos)
            pk.append(p)
            pos += len(p)
    data = np.zeros(pos + 64, np.uint8)
    for o, p in zip(offs, pk):
        data[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return data, np.array(offs, np.uint64), np.array([len(p) for p in pk], np.uint32)


@pytest.mark.parametrize("threshold", [None, 24, 1])
@pytest.mark.parametrize("v6", [False, True], ids=["icmp4", "icmp6"])
def test_sum_lengths_and_alignments(gpu_ctx, v6, threshold):
    """Messages of 8..41 bytes (odd lengths among them) and on both sides of the
    lane-group threshold, at every start alignment 0..15; with the threshold
    lowered the short messages take the 64-lane kernel too."""
    T = _lib.CTL_SUM_GROUP_BYTES
    lengths = list(range(8, 42)) + [1499, 1500, T - 1, T, T + 1, T + 15, T + 16, T + 1025]
    for good in (True, False):
        data, offs, caps = sum_batch(lengths, v6, good=good)
        m, _ = model_control(C.PARSER, data, offs, caps)
        h, _ = device_control(gpu_ctx, C.PARSER, data, offs, caps, threshold=threshold)
        assert_same_control(m, h, "sum")
        n = int(h["counts"][0])
        assert n == len(caps) == int(h["counts"][5]) and not np.any(h["records"][:n]["err"])
        st = h["records"][:n]["status"]
        assert np.all((st & 2) == 2) and (np.all(st & 4) if good else not np.any(st & 4))


def big_sum(h, pkt_index, msg, start=0):
    """The record of packet `pkt_index` against ComputeChecksum of `msg` worked out here."""
    total = start + sum(msg[i] << 8 | msg[i + 1] for i in range(0, len(msg) - 1, 2)) + \
        ((msg[-1] << 8) if len(msg) & 1 else 0)
    t = h["records"][int(h["verdict"][pkt_index])]
    assert int(t["contents_len"]) + int(t["payload_len"]) == len(msg)
    assert int(t["correct"]) == M.fold(((total & 0xffffffff) - int(t["checksum"])) & 0xffffffff)
    return total


def test_icmp4_sum_70000_bytes_of_ff(gpu_ctx):
    """70 000 bytes of 0xFF sum past 2^31. An IPv4 datagram cannot carry them (its
    TSO Length 0 form takes len & 0xffff, ip4.go:196-205, also in this batch),
    so the long message sits right behind Ethernet."""
    msg = b"\xff" * 70000
    tso = b"\xff" * 3000
    pk = [C.eth(msg, C.ET_ICMP4), C.eth(C.ip4(tso, 1, total=0)), dict(CASES)["icmp4_echo"]]
    data, offs, caps = pack(pk, pad=5)
    m, _ = model_control(C.PARSER, data, offs, caps)
    h, _ = device_control(gpu_ctx, C.PARSER, data, offs, caps)
    assert_same_control(m, h)
    assert big_sum(h, 0, msg) >= 1 << 31
    big_sum(h, 1, tso)


def test_icmp6_sum_140001_bytes_in_a_jumbogram(gpu_ctx):
    """A jumbogram whose ICMPv6 slice is 140 001 bytes, 0xFF behind the HopByHop
    header the slice starts at (ip6.go:249-256 keeps the payload there): the sum
    wraps 2^32 before the one fold (P8) and length >> 16 enters the pseudo-header."""
    size = 140001
    hop = C.hbh(58, b"\xc2\x04" + size.to_bytes(4, "big"))
    msg = hop + b"\xff" * (size - len(hop))
    pk = [C.eth(C.ip6(msg, 0, plen=0), 0x86dd), dict(CASES)["icmp6_echo_request"]]
    data, offs, caps = pack(pk, pad=3)
    m, _ = model_control(C.PARSER, data, offs, caps)
    h, _ = device_control(gpu_ctx, C.PARSER, data, offs, caps)
    assert_same_control(m, h)
    t = h["records"][int(h["verdict"][0])]
    assert int(t["kind"]) == _lib.CTL_ICMP6 and int(t["status"]) & 2
    start = M.sum_init(C.SRC6 + C.DST6, size)
    assert int(t["sum_init"]) == start and (size >> 16) == 2
    assert big_sum(h, 0, msg, start) >= 1 << 32


# ---- the composed DecodeBatch ---------------------------------------------------------------------
def real_parser(cfg=C.PARSER, ctx=None, **kw):
    p = control_parser(cfg, **kw)
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
    got, exp = res.levels[0][0].control, want["levels"][0][0]["control"]
    m = int(exp["counts"][0])
    assert np.array_equal(got["verdict"], exp["verdict"]) and got["records"].tobytes() == exp["records"][:m].tobytes()


def test_decode_batch_with_a_vxlan_level(gpu_ctx):
    c = dict(CASES)
    pk = [TC.over_udp(TC.vxlan(c["icmp6_echo_request"]), TC.VX), TC.over_udp(TC.geneve(c["arp_reply_padded_60"]), TC.GN),
          TC.over_ip(TC.gre(c["icmp4_echo"][14:])), c["icmp4_echo"], TC.over_udp(TC.vxlan(TC.inner_eth()), TC.VX),
          TC.over_udp(TC.vxlan(c["icmp6_neighbor_solicitation"]), TC.VX), c["plain_tcp"]] * 9
    want = M.compose(C.PARSER, pk, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 21, 57, 132]
    p = real_parser(C.PARSER, gpu_ctx, tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._controls[4].Identifier == 0xbeef and p._controls[2].VerifyChecksum()[1].Valid


def test_decode_layers_on_device_without_checksum(gpu_ctx):
    p = real_parser(ctx=gpu_ctx)
    c = dict(CASES)
    res = p.DecodeBatch(G.PacketBatch.from_packets([c["icmp4_bad_checksum"], c["icmp6_echo_request"]]), checksum=False)
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == [17, 20, 19, 2]
    err, r = p._controls[1].VerifyChecksum()  # no device sum: computed from the hydrated bytes
    assert err is None and not r.Valid and r.Actual == r.Correct ^ 0x0100
    assert res.Hydrate(1, decoded) is None
    assert p._controls[2].VerifyChecksum()[0].Error() == M.NO_NETWORK
    with pytest.raises(ValueError, match="fields=True"):
        p.DecodeBatch(G.PacketBatch.from_packets(PACKETS[:2]), fields=True)
