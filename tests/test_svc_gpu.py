"""gpk_svc_batch on the device against gpk_svc_batch_host and the model
(svc_model.py), byte for byte: every verdict, class boundary, index, message
record and entry descriptor, with the outputs pre-filled with 0xA5 so that a
stray write shows; the compaction at wave and block boundaries; the capacity
rule with the retry; a batch whose entries pass 2^16; the composed DecodeBatch,
one VXLAN level included. No tolerance anywhere."""
import numpy as np
import pytest
import torch

import configs
import ndp_model as NM
import ndpcases as NC
import svc_model as M
import svccases as C
from svcutil import (CASES, CONTROLS, GOLDEN_PACKETS, NAMES, PACKETS, assert_same_svc, corpus, device_arrays, svc_parser)
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition

pytestmark = pytest.mark.gpu
FILL32 = -1515870811  # 0xA5A5A5A5
ALL_ERRORS = set(range(_lib.SVC_ERR_FIRST, _lib.SVC_ERR_END)) | {_lib.ERR_PANIC_SLICE_B}


def dev(a):
    a = np.array(a)  # a writable copy
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def device_svc(ctx, cfg, data, offs, caps, entry_cap, kinds=M.ALL, svd=None, stream=None):
    """Decode with layouts and run the service pass on the device; outputs
    start as 0xA5 bytes. Returns (outputs as host arrays, decode results as
    host arrays)."""
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
               entries=torch.full((entry_cap * 8,), 0xA5, dtype=torch.uint8, device="cuda"))
    own = svd is None
    svd = svd or flows.ServiceDecoder(max(n, 1))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    svd.decode(ctx, d, o, c, rec, lay, p, entry_cap, kinds, out=out, stream=stream)
    torch.cuda.synchronize()
    if own:
        svd.close()
    r = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
             flows=fl.cpu().numpy().view(np.uint64), layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE))
    return device_arrays(out), r


def model_svc(cfg, data, offs, caps, entry_cap=None, kinds=M.ALL):
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    args = (cfg, data, offs, caps, ref["records"], ref["layouts"], kinds)
    if entry_cap is None:
        entry_cap = flows.ServiceDecoder.needed(M.svc(*args, entry_cap=0)["counts"])
    return M.svc(*args, entry_cap=entry_cap, fill=0xA5), ref


def host_svc(cfg, data, offs, caps, ref, entry_cap, kinds=M.ALL):
    return flows.ServiceDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], configs.device_parser(cfg),
                                            entry_cap, kinds, fill=0xA5)


def check(ctx, cfg, packets, align=1, pad=0, spare=3, kinds=M.ALL, **kw):
    """The device against the host entry and the model on whole arrays; the
    arena is `spare` entries longer than needed: the device must leave those
    at 0xA5."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    need = flows.ServiceDecoder.needed(host_svc(cfg, data, offs, caps, ref, 0, kinds)["counts"])
    cap = need + spare
    want = host_svc(cfg, data, offs, caps, ref, cap, kinds)
    m, _ = model_svc(cfg, data, offs, caps, cap, kinds)
    assert_same_svc(m, want, "host")
    h, r = device_svc(ctx, cfg, data, offs, caps, cap, kinds, **kw)
    configs.assert_same(r, ref, "decode")
    assert_same_svc(want, h, "device")  # whole arrays: what the host leaves at 0xA5 the device must not touch
    return want, h


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_cases_and_golden_packets(gpu_ctx, cfg):
    pk = PACKETS + GOLDEN_PACKETS + list(C.layers17())
    m, h = check(gpu_ctx, cfg, pk)
    assert int(m["counts"][1]) > 35 and int(m["counts"][2]) > 20
    assert int(h["verdict"][-1]) == _lib.SVC_UNKNOWN and int(h["verdict"][-2]) >= 0
    assert np.all(h["records"][int(h["counts"][0]):].view(np.uint8) == 0xA5)  # nothing written past the list
    assert {int(e) for e in h["records"][:int(h["counts"][0])]["err"]} - {0} == ALL_ERRORS


def test_kinds_on_the_device(gpu_ctx):
    for kinds in (1, 2, 4, 5):
        check(gpu_ctx, C.PARSER, PACKETS, kinds=kinds)


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_corpus(gpu_ctx, align, pad):
    check(gpu_ctx, C.PARSER, corpus(), align=align, pad=pad)


def class_samples():
    c = dict(CASES)
    # decoded and failed messages alternate, with 8, 0, 5, 0, 0 and 0 entries; and a plain packet
    return [c["dhcp4_discover_eight_options"], c["dhcp4_bad_magic"], c["dhcp6_solicit_five_options"], c["dhcp6_7_bytes"],
            c["ntp_48_bytes"], c["ntp_47_bytes"]], c["plain_udp"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1024, 1025])
def test_compaction_sizes(gpu_ctx, n):
    """Candidate counts around the wave (64) and the block (256), in three
    batch patterns: all candidates, every other packet, candidates last."""
    cand, plain = class_samples()
    for pattern in ("all", "alternating", "last"):
        if pattern == "all":
            pk = [cand[i % 6] for i in range(n)]
        elif pattern == "alternating":
            pk = [x for i in range(n) for x in (cand[i % 6], plain)]
        else:
            pk = [plain] * 300 + [cand[i % 6] for i in range(n)]
        m, h = check(gpu_ctx, C.PARSER, pk)
        assert int(h["counts"][0]) == n
        if n >= 64:
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
    svd = flows.ServiceDecoder(600)
    for n in (600, 5, 300):
        pk = [cand[i % 6] if i % 3 else plain for i in range(n)]
        check(gpu_ctx, C.PARSER, pk, svd=svd)
    with pytest.raises(_lib.GpkError):
        data, offs, caps = pack([plain] * 601)
        device_svc(gpu_ctx, C.PARSER, data, offs, caps, 4, svd=svd)
    svd.close()


def test_stream_and_device_are_left_alone(gpu_ctx):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    before = torch.cuda.current_device()
    svd = flows.ServiceDecoder(len(PACKETS), before)
    check(gpu_ctx, C.PARSER, PACKETS, svd=svd, stream=torch.cuda.Stream())
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = flows.ServiceDecoder(16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    svd.close()
    assert torch.cuda.current_device() == before


def test_capacity_rule_and_retry(gpu_ctx):
    """Exact fit, one entry short, capacity 0, half: whole messages or nothing,
    nothing at or past the capacity; then decode_all's retry from capacities of
    0 and 1."""
    pk = PACKETS * 2
    data, offs, caps = pack(pk)
    full, ref = model_svc(C.PARSER, data, offs, caps)
    need = len(full["entries"])
    assert need > 600
    for cap in (need, need - 1, 0, 1, need // 2):
        m, _ = model_svc(C.PARSER, data, offs, caps, cap)
        assert_same_svc(m, host_svc(C.PARSER, data, offs, caps, ref, cap), "host cap %d" % cap)
        h, _ = device_svc(gpu_ctx, C.PARSER, data, offs, caps, cap)
        assert_same_svc(m, h, "cap %d" % cap)
        assert int(h["counts"][3]) == int(cap < need) and flows.ServiceDecoder.needed(h["counts"]) == need
    p = configs.device_parser(C.PARSER)
    n = len(caps)
    d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
    o, c = dev(offs), dev(caps)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(p, d, o, c, rec, torch.zeros(2 * n, dtype=torch.int32, device="cuda"),
                          torch.zeros(3 * n, dtype=torch.int64, device="cuda"), lay)
    svd = flows.ServiceDecoder(n)
    for first in (0, 1):
        out = svd.decode_all(gpu_ctx, d, o, c, rec, lay, p, entry_cap=first)
        torch.cuda.synchronize()
        assert not int(out["counts"][3].item())
        assert out["entries"].cpu().numpy().tobytes() == full["entries"].tobytes()
        m = int(full["counts"][0])
        assert out["records"].cpu().numpy()[:m * 64].tobytes() == full["records"][:m].tobytes()
    svd.close()


def test_pad_messages_pass_two_to_the_16_entries(gpu_ctx):
    """1 Ki messages of 300 Pad bytes: the pass's worst case, one entry per
    byte, 307 200 entries in one call; entry0 runs past 2^16. The model decodes
    one message; the batch's arrays follow from it, since offsets are relative
    to the packet: the same 300 entries 1024 times, entry0 = 300 j."""
    n, per, spare = 1024, 300, 3
    pk = [dict(CASES)["dhcp4_300_pads"]] * n
    data, offs, caps = pack(pk)
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    one, _ = model_svc(C.PARSER, data[:int(offs[1])], offs[:1], caps[:1])
    assert int(one["records"][0]["nentries"]) == per == len(one["entries"])
    assert np.array_equal(one["entries"]["off"], C.HDR + 241 + np.arange(per, dtype=np.uint32))
    need = per * n
    records = np.repeat(one["records"][:1], n)
    records["entry0"] = per * np.arange(n, dtype=np.uint64)
    fill = np.empty(spare, _lib.SVC_ENTRY_DTYPE)
    fill.view(np.uint8)[:] = 0xA5
    m = dict(verdict=np.arange(n, dtype=np.int32), class_start=np.array([0, n, n], np.uint32),
             index=np.arange(n, dtype=np.uint32), records=records,
             counts=np.array([n, n, 0, 0, need, 0, 0, 0], np.uint32), entries=np.concatenate([np.tile(one["entries"], n), fill]))
    assert_same_svc(m, host_svc(C.PARSER, data, offs, caps, ref, need + spare), "host")
    h, _ = device_svc(gpu_ctx, C.PARSER, data, offs, caps, need + spare)
    assert_same_svc(m, h, "pads")
    assert flows.ServiceDecoder.needed(h["counts"]) == need > 1 << 16
    assert [int(x) for x in h["records"]["entry0"][[0, 1, 219, 1023]]] == [0, 300, 65700, 306900]


def test_argument_faults(gpu_ctx):
    data, offs, caps = pack(PACKETS[:4])
    n = len(caps)
    p = configs.device_parser(C.PARSER)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    svd = flows.ServiceDecoder(n)
    try:
        with pytest.raises(_lib.GpkError):  # data not 16-byte aligned
            d = dev(np.concatenate([np.zeros(1, np.uint8), data, np.zeros(32, np.uint8)]))[1:]
            svd.decode(gpu_ctx, d, dev(offs), dev(caps), rec, lay, p, 4)
        d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
        for kinds in (0, 8, 15):
            with pytest.raises(_lib.GpkError):
                svd.decode(gpu_ctx, d, dev(offs), dev(caps), rec, lay, p, 4, kinds)
    finally:
        svd.close()
    with pytest.raises(_lib.GpkError):
        flows.ServiceDecoder(0)
    with pytest.raises(_lib.GpkError):
        flows.ServiceDecoder(1 << 28)


# ---- the composed DecodeBatch ---------------------------------------------------------------------
def real_parser(cfg=C.PARSER, ctx=None, **kw):
    p = svc_parser(cfg, **kw)
    p._host_decoder = None  # the device decodes
    p._ctx = ctx
    return p


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_decode_batch_composed(gpu_ctx, cfg):
    pk = PACKETS + GOLDEN_PACKETS + corpus()[:700]
    want = M.compose(cfg, pk)
    p = real_parser(cfg, gpu_ctx)
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    assert isinstance(res, G.TunnelBatchResult) and len(res.levels) == 1
    check_composition(res, want, len(pk))
    got, exp = res.levels[0][0].svc, want["levels"][0][0]["svc"]
    m = int(exp["counts"][0])
    assert np.array_equal(got["verdict"], exp["verdict"]) and got["records"].tobytes() == exp["records"][:m].tobytes()
    assert got["entries"].tobytes() == exp["entries"].tobytes()
    decoded = []
    i = NAMES.index("dhcp4_discover_eight_options")
    assert res.Hydrate(i, decoded) is None and [int(t) for t in decoded] == [17, 20, 45, 118]
    assert [int(o.Type) for o in p._svcs[_lib.SVC_DHCP4].Options] == [53, 61, 12, 60, 50, 55, 57, 51]
    assert len(res.Service(i)[1]) == 8
    with pytest.raises(ValueError, match="fields=True"):
        p.DecodeBatch(G.PacketBatch.from_packets(pk[:4]), fields=True)


def test_decode_batch_without_the_layers_is_the_ndp_pass(gpu_ctx):
    """A parser that holds the control and NDP layers only runs what it ran before."""
    pk = PACKETS + corpus()[:256]
    want = NM.compose(C.PARSER, pk)
    res = real_parser(C.PARSER, gpu_ctx, extra=L.NDP_LAYERS + CONTROLS).DecodeBatch(G.PacketBatch.from_packets(pk))
    check_composition(res, want, len(pk))
    assert all(part.svc is None for lvl in res.levels for part in lvl)
    assert res.Err(NAMES.index("ntp_48_bytes")).Error() == "No decoder for layer type NTP"


def test_decode_batch_with_a_vxlan_level(gpu_ctx):
    c, nc = dict(CASES), dict(NC.quirk_cases()[0])
    pk = [C.over_udp(C.vxlan(c["dhcp4_ack"]), C.VX), c["dhcp4_discover_eight_options"], nc["ra_three_options"],
          C.over_udp(C.vxlan(c["dhcp6_7_bytes"]), C.VX), c["ntp_48_bytes"], c["plain_udp"],
          C.over_udp(C.vxlan(c["ntp_47_bytes"]), C.VX), C.over_udp(C.vxlan(nc["ns_one_option"]), C.VX)] * 9
    want = M.compose(C.PARSER, pk, base=NM.compose(C.PARSER, pk, control_kinds=15, tunnel_kinds=7))
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 20, 45, 118]
    p = real_parser(C.PARSER, gpu_ctx, extra=L.SVC_LAYERS + L.NDP_LAYERS + CONTROLS, tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._svcs[_lib.SVC_DHCP4].YourClientIP == bytes([10, 0, 0, 99]) and p._tunnels[2].VNI == 0x123456
