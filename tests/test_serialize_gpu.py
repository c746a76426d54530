"""gpk_serialize_batch (the write kernel of include/gpk_serialize.h) against the
model (serialize_model.py): every byte of out[:counts[1]], out_offsets,
out_caplens, status, err_args and counts, with a canary before and after, under
the four option sets and both group sizes of the write kernel (forced through
gpk_serialize_opts.group), on the shapes of serializecases.py; then a
20 000-packet C4-mix batch decoded on the device, m = 0, order NULL / a
permutation / a selection with repeats, overflow at three cut points, and the
round trip decode -> serialize {} -> decode."""
import numpy as np
import pytest

import serialize_model as M
import serializecases as C
from gopacket_amd import _lib, engine, gopacket as G, synth
from gopacket_amd.flows import Serializer

pytestmark = pytest.mark.gpu

OPTS = [(0, 0), (1, 0), (0, 1), (1, 1)]
GROUPS = [16, 64]
FILL = 0xA5
_dev, _want, _cut = {}, {}, {}


def dev(which):
    import torch
    if which not in _dev:
        b = C.build(which)
        _dev[which] = dict(d=torch.from_numpy(b["data"]).cuda(), o=torch.from_numpy(b["offsets"].astype(np.int64)).cuda(),
                           c=torch.from_numpy(b["caplens"].astype(np.int32)).cuda(),
                           l=torch.from_numpy(b["layouts"].view(np.uint8).copy()).cuda(),
                           f=torch.from_numpy(b["fields"].view(np.uint8).copy()).cuda())
    return _dev[which]


def want(which, fix, csum, order=None, key=None):
    k = (which, fix, csum, key)
    if k not in _want:
        b = C.build(which)
        _want[k] = M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], order, fix, csum)
    return _want[k]


@pytest.fixture(scope="module")
def ser(gpu_ctx):
    s = Serializer(1 << 16, device=0)
    yield s
    s.close()


def run(ser, t, fix, csum, group, order=None, cap=None, base=0, need=None):
    """Serialize into a canary-filled buffer at byte offset `base`; returns host arrays and the whole buffer."""
    import torch
    n = int(need if cap is None else cap)
    buf = torch.full((base + n + 64,), FILL, dtype=torch.uint8, device="cuda")
    od = None if order is None else torch.from_numpy(order.astype(np.int32)).cuda()
    r = ser.serialize(t["d"], t["o"], t["c"], t["l"], t["f"], od, fix, csum, out=buf[base:], out_cap=n, group=group)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in r.items() if k != "out"}
    got["offsets"] = got["offsets"].view(np.uint64)
    got["caplens"] = got["caplens"].view(np.uint32)
    got["err_args"] = got["err_args"].view(np.uint32)
    got["counts"] = got["counts"].view(np.uint64)
    whole = buf.cpu().numpy()
    got["out"] = whole[base:]
    return got, whole


def same(got, whole, ref, base, cap=None):
    assert np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["offsets"], ref["offsets"]) and np.array_equal(got["caplens"], ref["caplens"])
    assert np.array_equal(got["err_args"], ref["err_args"])
    total = int(ref["counts"][1])
    end = total if cap is None else cap
    if cap is None:
        assert np.array_equal(got["out"][:total], ref["out"])
    else:  # a packet that does not end inside cap is not written at all
        exp = np.full(cap, FILL, np.uint8)
        for j in range(len(ref["status"])):
            lo, hi = int(ref["offsets"][j]), int(ref["offsets"][j + 1])
            if hi <= cap:
                exp[lo:hi] = ref["out"][lo:hi]
        assert np.array_equal(got["out"][:cap], exp)
    assert (whole[:base] == FILL).all() and (whole[base + end:] == FILL).all()  # the canary on both sides


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("fix,csum", OPTS)
@pytest.mark.parametrize("which,base", [("cases", 0), ("cases", 5), ("tails", 0), ("tails", 9)])
def test_device_matches_model(ser, which, base, fix, csum, group):
    ref = want(which, fix, csum)
    got, whole = run(ser, dev(which), fix, csum, group, base=base, need=int(ref["counts"][1]))
    same(got, whole, ref, base)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("fix,csum", OPTS)
def test_output_base_offsets(ser, fix, csum, group):
    """every output base offset 0..15"""
    ref = want("tails", fix, csum)
    for base in range(16):
        got, whole = run(ser, dev("tails"), fix, csum, group, base=base, need=int(ref["counts"][1]))
        same(got, whole, ref, base)


@pytest.mark.parametrize("group", [0] + GROUPS)
@pytest.mark.parametrize("fix,csum", OPTS)
def test_order_m0_overflow(ser, fix, csum, group):
    b = C.build("cases")
    n = len(b["caplens"])
    small = np.nonzero(b["caplens"] < 4000)[0].astype(np.uint32)
    perm = np.random.default_rng(7).permutation(small).astype(np.uint32)
    rep = np.array([3, 3, 70, n, 3, 0, n + 5, 70], np.uint32)
    for key, order in (("perm", perm), ("rep", rep), ("m0", np.zeros(0, np.uint32))):
        ref = want("cases", fix, csum, order, key)
        got, whole = run(ser, dev("cases"), fix, csum, group, order=order, base=3, need=int(ref["counts"][1]))
        same(got, whole, ref, 3)
    order = small[:40]
    full = want("cases", fix, csum, order, "first40")
    total = int(full["counts"][1])
    for cap in (0, int(full["offsets"][17]) + 1, total - 1):
        k = (fix, csum, cap)
        if k not in _cut:
            _cut[k] = M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], order, fix, csum,
                                        out_cap=cap)
        ref = _cut[k]
        got, whole = run(ser, dev("cases"), fix, csum, group, order=order, cap=cap, base=1)
        assert int(ref["counts"][3]) == 1
        same(got, whole, ref, 1, cap=cap)


@pytest.fixture(scope="module")
def c4(gpu_ctx):
    """20 000 packets of the C4 mix, decoded on the device with layouts and fields"""
    import torch
    n = 20000
    decoders = [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP,
                _lib.DEC_UDP, _lib.DEC_PAYLOAD]
    ctx = engine.Context(0)
    p = engine.ParserConfig(17, decoders)
    d, o, c = synth.device_batch(synth.C4_IMIX, 0, n)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    f = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    ctx.decode_device_fields(p, d, o, c, rec, err, fl, f, layouts=lay, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    host = dict(data=d.cpu().numpy(), offsets=o.cpu().numpy().view(np.uint64), caplens=c.cpu().numpy().view(np.uint32),
                layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE), fields=f.cpu().numpy().view(_lib.FIELDS_DTYPE))
    return dict(ctx=ctx, p=p, t=dict(d=d, o=o, c=c, l=lay, f=f), host=host, rec=rec, err=err, fl=fl)


@pytest.mark.parametrize("fix,csum", OPTS)
def test_c4_mix(ser, c4, fix, csum):
    h = c4["host"]
    ref = M.serialize_batch(h["data"], h["offsets"], h["caplens"], h["layouts"], h["fields"], None, fix, csum)
    assert int(ref["counts"][2]) == 0
    for group in GROUPS:
        got, whole = run(ser, c4["t"], fix, csum, group, base=0, need=int(ref["counts"][1]))
        same(got, whole, ref, 0)


def test_roundtrip_decodes_the_same(ser, c4):
    """decode -> serialize {} -> decode: the same records and fields for packets with valid checksums"""
    import torch
    h, n = c4["host"], 20000
    # the premise, with the model on the CPU: {} gives every packet's own bytes back (a short frame padded to 60)
    ref = M.serialize_batch(h["data"], h["offsets"], h["caplens"], h["layouts"], h["fields"], None, 0, 0)
    assert np.array_equal(ref["caplens"], h["caplens"]) and not ref["status"].any()
    for j in range(0, n, 97):
        a, ln = int(h["offsets"][j]), int(h["caplens"][j])
        assert bytes(ref["out"][int(ref["offsets"][j]):int(ref["offsets"][j + 1])]) == bytes(h["data"][a:a + ln])
    res = G.SerializeBatch(G.SerializeOptions(), c4["t"]["d"], c4["t"]["o"], c4["t"]["c"], c4["t"]["l"], c4["t"]["f"])
    rec2 = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    f2 = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
    lay2 = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    c4["ctx"].decode_device_fields(c4["p"], res["out"], res["offsets"][:n].contiguous(), res["caplens"], rec2,
                                   torch.zeros_like(c4["err"]), torch.zeros_like(c4["fl"]), f2, layouts=lay2,
                                   stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(res["caplens"], c4["t"]["c"]) and int(res["counts"][2].item()) == 0
    assert torch.equal(rec2, c4["rec"]) and torch.equal(f2, c4["t"]["f"]) and torch.equal(lay2, c4["t"]["l"])


def test_python_device_path_raises(ser):
    t = dev("cases")
    with pytest.raises(G.SerializeError) as e:
        G.SerializeBatch(G.SerializeOptions(FixLengths=True), t["d"], t["o"], t["c"], t["l"], t["f"], raise_errors=True)
    ref = want("cases", 1, 0)
    j = int(np.nonzero(ref["status"])[0][0])
    assert e.value.packet == j and e.value.status == int(ref["status"][j])
