"""gpk_tls_batch on the device against the model (tls_model.py), byte for byte:
every verdict, class boundary, index, message record, record entry, hello
entry and server name byte, with the outputs pre-filled so that a stray write
shows; the compaction at wave and block boundaries; the capacity rules with
the retry; the composed DecodeBatch, one VXLAN level included. No tolerance
anywhere. Messages stay at or under 1500 bytes."""
import numpy as np
import pytest
import torch

import configs
import tls_model as M
import tlscases as C
import tunnelcases as TC
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tlsutil import GOLDEN, assert_same_tls, golden_packet, tls_parser
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


def upload_and_decode(ctx, cfg, data, offs, caps):
    n = len(caps)
    p = configs.device_parser(cfg)
    d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
    o, c = dev(offs), dev(caps)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    ctx.decode_device(p, d, o, c, rec, err, fl, lay)
    return p, d, o, c, rec, err, fl, lay


def device_tls(ctx, cfg, data, offs, caps, caps3, tld=None, stream=None):
    """Decode with layouts and run the TLS pass on the device; outputs start
    as 0xA5 bytes. caps3: (rec_cap, hello_cap, sni_cap). Returns (outputs as
    host arrays, decode results as host arrays)."""
    n = len(caps)
    p, d, o, c, rec, err, fl, lay = upload_and_decode(ctx, cfg, data, offs, caps)
    out = dict(verdict=torch.full((n,), FILL32, dtype=torch.int32, device="cuda"),
               class_start=torch.full((3,), FILL32, dtype=torch.int32, device="cuda"),
               index=torch.full((n,), FILL32, dtype=torch.int32, device="cuda"),
               records=torch.full((n * 80,), 0xA5, dtype=torch.uint8, device="cuda"),
               counts=torch.full((12,), FILL32, dtype=torch.int32, device="cuda"),
               recs=torch.full((caps3[0] * 16,), 0xA5, dtype=torch.uint8, device="cuda"),
               hellos=torch.full((caps3[1] * 64,), 0xA5, dtype=torch.uint8, device="cuda"),
               snis=torch.full((caps3[2],), 0xA5, dtype=torch.uint8, device="cuda"))
    own = tld is None
    tld = tld or flows.TLSDecoder(max(n, 1))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    tld.decode(ctx, d, o, c, rec, lay, p, *caps3, out=out, stream=stream)
    torch.cuda.synchronize()
    if own:
        tld.close()
    h = dict(verdict=out["verdict"].cpu().numpy(), class_start=out["class_start"].cpu().numpy().view(np.uint32),
             index=out["index"].cpu().numpy().view(np.uint32), records=out["records"].cpu().numpy().view(_lib.TLS_DTYPE),
             counts=out["counts"].cpu().numpy().view(np.uint32), recs=out["recs"].cpu().numpy().view(_lib.TLS_REC_DTYPE),
             hellos=out["hellos"].cpu().numpy().view(_lib.TLS_HELLO_DTYPE), snis=out["snis"].cpu().numpy())
    r = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
             flows=fl.cpu().numpy().view(np.uint64), layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE))
    return h, r


def model_tls(cfg, data, offs, caps, caps3=(None, None, None)):
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    return M.tls(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], *caps3, fill=0xA5), ref


def check(ctx, cfg, packets, align=1, pad=0, spare=(3, 2, 5), **kw):
    """The device against the model on whole arrays; the arenas are `spare`
    entries and bytes longer than needed: the device must leave those at 0xA5."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    exact, _ = model_tls(cfg, data, offs, caps)
    caps3 = (len(exact["recs"]) + spare[0], len(exact["hellos"]) + spare[1], len(exact["snis"]) + spare[2])
    m, ref = model_tls(cfg, data, offs, caps, caps3)
    h, r = device_tls(ctx, cfg, data, offs, caps, caps3, **kw)
    configs.assert_same(r, ref, "decode")
    assert_same_tls(m, h, "device")  # whole arrays: what the model leaves at 0xA5 the device must not touch
    return m, h


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_cases_and_golden_packets(gpu_ctx, cfg):
    """Every case and the harvested vectors. The longest walk is
    appdata_300_empty: 300 records in one lane."""
    pk = PACKETS + [golden_packet(v)[0] for v in GOLDEN] + list(C.layers17())
    m, h = check(gpu_ctx, cfg, pk)
    assert int(m["counts"][1]) > 40 and int(m["counts"][2]) > 40
    assert int(h["verdict"][-1]) == _lib.TLS_UNKNOWN
    assert np.all(h["records"][int(h["counts"][0]):].view(np.uint8) == 0xA5)  # nothing written past the list
    errs = {int(e) for e in h["records"][:int(h["counts"][0])]["err"]}
    assert errs >= set(M.ALL_ERRORS)
    assert (pk.index(dict(CASES)["hello_with_sni"]), b"example.com") in M.snis(h)


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_fuzz_corpus(gpu_ctx, fuzz, align, pad):
    check(gpu_ctx, C.PARSER, fuzz, align=align, pad=pad)


def class_samples():
    c = dict(CASES)
    # an OK and a failed message alternate, with different record, hello and name sizes; and a plain packet
    return [c["two_hellos"], c["length_one_short"], c["appdata_2"], c["sni_hostname_length_fff8_panics"], c["four_kinds"],
            c["hello_spills_into_next_record"]], c["plain_tcp_port_80"]


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


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
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
    tld = flows.TLSDecoder(600)
    for n in (600, 5, 300):
        pk = [cand[i % 6] if i % 3 else plain for i in range(n)]
        check(gpu_ctx, C.PARSER, pk, tld=tld)
    with pytest.raises(_lib.GpkError):
        data, offs, caps = pack([plain] * 601)
        device_tls(gpu_ctx, C.PARSER, data, offs, caps, (4, 4, 4), tld=tld)
    tld.close()


def test_stream_and_device_are_left_alone(gpu_ctx):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    before = torch.cuda.current_device()
    tld = flows.TLSDecoder(len(PACKETS), before)
    check(gpu_ctx, C.PARSER, PACKETS, tld=tld, stream=torch.cuda.Stream())
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = flows.TLSDecoder(16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    tld.close()
    assert torch.cuda.current_device() == before


def test_capacity_rules_and_retry(gpu_ctx):
    """Exact fit, one short and zero in each arena separately, half: whole
    messages or nothing, nothing at or past a capacity; then decode_all's
    retry from capacities of 1."""
    cand, plain = class_samples()
    pk = (cand + [plain, dict(CASES)["sni_absent"], dict(CASES)["ccs_message_1"]]) * 8
    data, offs, caps = pack(pk)
    full, _ = model_tls(C.PARSER, data, offs, caps)
    need = (len(full["recs"]), len(full["hellos"]), len(full["snis"]))
    trials = [need, (0, 0, 0), tuple(x // 2 for x in need)]
    for k in range(3):
        trials += [tuple(x - (j == k) for j, x in enumerate(need)), tuple(0 if j == k else x for j, x in enumerate(need))]
    for caps3 in trials:
        m, _ = model_tls(C.PARSER, data, offs, caps, caps3)
        h, _ = device_tls(gpu_ctx, C.PARSER, data, offs, caps, caps3)
        assert_same_tls(m, h, "caps %r" % (caps3,))
        assert int(h["counts"][3]) == int(any(a < b for a, b in zip(caps3, need)))
        assert flows.TLSDecoder.needed(h["counts"]) == need
    p, d, o, c, rec, _, _, lay = upload_and_decode(gpu_ctx, C.PARSER, data, offs, caps)
    tld = flows.TLSDecoder(len(caps))
    out = tld.decode_all(gpu_ctx, d, o, c, rec, lay, p, rec_cap=1, hello_cap=1, sni_cap=1)
    torch.cuda.synchronize()
    tld.close()
    assert not int(out["counts"][3].item())
    for k in ("recs", "hellos", "snis"):
        assert out[k].cpu().numpy().tobytes() == full[k].tobytes(), k


def test_argument_faults(gpu_ctx):
    """Return codes only: every bad call is refused before a kernel is launched."""
    data, offs, caps = pack(PACKETS[:4])
    n = len(caps)
    p = configs.device_parser(C.PARSER)
    tld = flows.TLSDecoder(n)
    try:
        rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.GpkError):  # data not 16-byte aligned
            d = dev(np.concatenate([np.zeros(1, np.uint8), data, np.zeros(32, np.uint8)]))[1:]
            tld.decode(gpu_ctx, d, dev(offs), dev(caps), rec, lay, p, 4, 4, 4)
        d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
        good = tld.decode(gpu_ctx, d, dev(offs), dev(caps), rec, lay, p, 8, 4, 64)
        torch.cuda.synchronize()
        for key in ("recs", "hellos", "records"):  # an entry array that is not 8-byte aligned
            bad = dict(good)
            bad[key] = torch.zeros(good[key].numel() + 8, dtype=torch.uint8, device="cuda")[4:]
            with pytest.raises(_lib.GpkError):
                tld.decode(gpu_ctx, d, dev(offs), dev(caps), rec, lay, p, 8, 4, 64, out=bad)
    finally:
        tld.close()
    with pytest.raises(_lib.GpkError):
        flows.TLSDecoder(0)
    with pytest.raises(_lib.GpkError):
        flows.TLSDecoder(1 << 28)


# ---- the composed DecodeBatch ---------------------------------------------------------------------
def real_parser(cfg=C.PARSER, ctx=None, **kw):
    p = tls_parser(cfg, **kw)
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
    got, exp = res.levels[0][0].tls, want["levels"][0][0]["tls"]
    m = int(exp["counts"][0])
    assert np.array_equal(got["verdict"], exp["verdict"]) and got["records"].tobytes() == exp["records"][:m].tobytes()
    for k in ("recs", "hellos", "snis"):
        assert got[k].tobytes() == exp[k].tobytes(), k
    assert res.SNIs() == M.snis(exp) and len(res.SNIs()) > 50


def test_decode_batch_with_and_without_the_layer(gpu_ctx):
    c = dict(CASES)
    pk = [bytes.fromhex(GOLDEN[0]["hex"]), c["appdata_2"], c["registered_port_8443"]]
    p = real_parser(ctx=gpu_ctx)
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == [17, 20, 44, 140]
    assert p._tls.Handshake[0].ClientHello.SNI == b"www.google.com" and res.SNIs() == [(0, b"www.google.com")]
    assert all([int(t) for t in res.Decoded(i)] == [17, 20, 44, 140] and res.Err(i) is None for i in range(3))
    q = real_parser(ctx=gpu_ctx, extra=())
    plain = q.DecodeBatch(G.PacketBatch.from_packets(pk), layouts=True)
    assert not isinstance(plain, G.TunnelBatchResult)
    assert [int(t) for t in plain.Decoded(0)] == [17, 20, 44] and plain.Err(0).Error() == "No decoder for layer type TLS"
    with pytest.raises(ValueError, match="fields=True"):
        p.DecodeBatch(G.PacketBatch.from_packets(pk), fields=True)


def test_decode_batch_with_a_vxlan_level(gpu_ctx):
    c = dict(CASES)
    pk = [TC.over_udp(TC.vxlan(c["hello_with_sni"]), TC.VX), c["appdata_2"], TC.over_udp(TC.vxlan(TC.inner_eth()), TC.VX),
          TC.over_udp(TC.vxlan(c["sni_hostname_length_ffff_panics"]), TC.VX), c["plain_tcp_port_80"],
          TC.over_udp(TC.vxlan(c["length_one_short"]), TC.VX)] * 9
    want = M.compose(C.PARSER, pk, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 20, 44, 140]
    p = real_parser(C.PARSER, gpu_ctx, tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = p.DecodeBatch(G.PacketBatch.from_packets(pk))
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._tls.Handshake[0].ClientHello.SNI == b"example.com" and p._tunnels[2].VNI == 0x123456
    assert res.SNIs() == [(i, b"example.com") for i in range(0, len(pk), 6)]
