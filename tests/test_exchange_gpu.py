"""gpk_pack_batch (the send side of the flow exchange) against numpy on
fuzzed and synthetic packets, every byte: repeats, empty and single
selections, zero-length packets, packets over 64 KiB, output past 4 GiB and
the argument contract; exchange_packets over RCCL with one rank on the
GPU (all-to-alls of device tensors through the nccl backend)."""
import os
import socket

import numpy as np
import pytest

import pktutil
from gopacket_amd import flows, shard, synth

pytestmark = pytest.mark.gpu


def upload(data, off, cap):
    import torch
    return (torch.from_numpy(data).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
            torch.from_numpy(cap.astype(np.int32)).cuda())


def expected_pack(data, off, cap, order):
    """numpy: (one buffer of the packets `order` back to back, offsets, caplens)."""
    caps = cap[order].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64) if len(order) else np.zeros(0, np.int64)
    parts = [data[int(off[i]):int(off[i]) + int(cap[i])] for i in order]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), offs, caps.astype(np.int32)


def test_pack_batch_matches_numpy(gpu_ctx):
    import torch
    pk = pktutil.fuzz_packets(77, 5000) + [b""] * 3
    data, off, cap = pktutil.pack(pk, align=7, pad=5)
    d, o, c = upload(data, off, cap)
    rng = np.random.default_rng(2)
    order = rng.permutation(len(pk))[:4000].astype(np.int32)
    od, oo, oc = flows.pack_batch(d, o, c, torch.from_numpy(order).cuda())
    torch.cuda.synchronize()
    od, oo, oc = od.cpu().numpy(), oo.cpu().numpy(), oc.cpu().numpy()
    assert np.array_equal(oc, cap[order].astype(np.int32))
    assert np.array_equal(oo, np.concatenate([[0], np.cumsum(cap[order], dtype=np.int64)[:-1]]))
    want, _, _ = expected_pack(data, off, cap, order)
    assert np.array_equal(od[:len(want)], want)  # every packet's bytes


GUARD = 0xA5


def pack_direct(d, o, c, order):
    """gpk_pack_batch through the C ABI into outputs this test allocates and
    pre-fills: out_data has exactly the selected bytes plus 16 spare bytes.
    -> numpy (out_data, out_offsets, out_caplens), whole arrays."""
    import ctypes

    import torch
    from gopacket_amd import _lib
    m = len(order)
    total = int(c.cpu().numpy()[order].sum()) if m else 0
    od = torch.full((total + 16,), GUARD, dtype=torch.uint8, device="cuda")
    oo = torch.full((m + 1,), -7, dtype=torch.int64, device="cuda")
    oc = torch.full((m + 1,), -7, dtype=torch.int32, device="cuda")
    ot = torch.from_numpy(np.asarray(order, np.int32)).cuda() if m else None
    b = _lib.Batch(d.data_ptr(), o.data_ptr(), c.data_ptr(), o.numel(), d.numel())
    _lib.check(_lib.lib().gpk_pack_batch(ctypes.byref(b), ot.data_ptr() if m else None, m, od.data_ptr(),
                                         oo.data_ptr(), oc.data_ptr(), None))
    torch.cuda.synchronize()
    return od.cpu().numpy(), oo.cpu().numpy(), oc.cpu().numpy()


@pytest.mark.parametrize("align,pad", [(1, 0), (7, 5)])
def test_pack_batch_order_shapes(gpu_ctx, align, pad):
    """Empty and single selections, identity, reversed, every packet three
    times in a row and one packet m times (the header allows repeats: the
    capture writer and the TCP assembler rely on them), runs of zero-length
    packets at the start, in the middle and at the end, a 70 000-byte and a
    262 144-byte packet among small ones. Every output byte is compared; the
    entries past m and the 16 bytes after the last packet stay untouched."""
    rng = np.random.default_rng(44)
    pk = pktutil.fuzz_packets(78, 700)
    big1 = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    big2 = bytes(rng.integers(0, 256, 262144, dtype=np.uint8))
    pk = [b""] + pk[:300] + [big1, b"", b""] + pk[300:] + [big2, b"tail", b""]
    n = len(pk)
    zeros = [i for i, p in enumerate(pk) if not p]
    assert len(zeros) >= 4 and max(len(p) for p in pk) == 262144
    data, off, cap = pktutil.pack(pk, align=align, pad=pad)
    d, o, c = upload(data, off, cap)
    ident = np.arange(n)
    some = rng.permutation(n)[:50]
    orders = {
        "m = 0": np.zeros(0, np.int64), "m = 1": np.array([5]), "m = 1, empty packet": np.array([zeros[0]]),
        "m = 1, the largest": np.array([n - 3]), "identity": ident, "reversed": ident[::-1],
        "each three times": np.repeat(ident[::5], 3), "one packet 500 times": np.full(500, 7),
        "the 70 000-byte packet 9 times": np.full(9, 301),
        "zero-length runs": np.concatenate([zeros, zeros, some, zeros, zeros[:2], some[::-1], zeros, zeros]),
        "only zero-length": np.array(zeros * 3),
    }
    assert len(pk[301]) == 70000
    for name, order in orders.items():
        m = len(order)
        want, woff, wcap = expected_pack(data, off, cap, order)
        od, oo, oc = pack_direct(d, o, c, order)
        assert np.array_equal(oc[:m], wcap) and oc[m] == -7, name
        assert np.array_equal(oo[:m], woff) and oo[m] == -7, name
        assert len(od) == len(want) + 16 and np.array_equal(od[:len(want)], want), name
        assert np.all(od[len(want):] == GUARD), name


def test_pack_batch_output_past_4_GiB(gpu_ctx):
    """One 262 144-byte packet selected 16 400 times: 4.3 GB of output, the
    offsets widened to 64 bits in the scan. Offsets and caplens are compared on
    the device for every j, the bytes for the packets on either side of 2^32
    (16 384 * 262 144) and at both ends; nothing large is read back."""
    import torch
    L, m = 262144, 16400
    rng = np.random.default_rng(45)
    pk = [b"small", bytes(rng.integers(0, 256, L, dtype=np.uint8)), b"other"]
    data, off, cap = pktutil.pack(pk)
    d, o, c = upload(data, off, cap)
    order = torch.ones(m, dtype=torch.int32, device="cuda")
    od, oo, oc = flows.pack_batch(d, o, c, order, total_bytes=L * m)
    torch.cuda.synchronize()
    assert torch.equal(oo, torch.arange(m, dtype=torch.int64, device="cuda") * L)
    assert int(oo[-1]) > 1 << 32 and bool((oc == L).all())
    src = d[int(off[1]):int(off[1]) + L]
    for j in (0, 16383, 16384, 16399):
        assert torch.equal(od[j * L:(j + 1) * L], src), j
    del od, oo, oc
    torch.cuda.empty_cache()


def test_pack_batch_argument_contract(gpu_ctx):
    """m >= 2^31 and null arrays with m > 0 return GPK_EINVAL; m = 0 needs no arrays."""
    import ctypes

    import torch
    from gopacket_amd import _lib
    data, off, cap = pktutil.pack([b"abc", b"defg"])
    d, o, c = upload(data, off, cap)
    order = torch.zeros(4, dtype=torch.int32, device="cuda")
    od = torch.zeros(64, dtype=torch.uint8, device="cuda")
    oo = torch.zeros(4, dtype=torch.int64, device="cuda")
    oc = torch.zeros(4, dtype=torch.int32, device="cuda")
    b = _lib.Batch(d.data_ptr(), o.data_ptr(), c.data_ptr(), 2, d.numel())
    good = [order.data_ptr(), 2, od.data_ptr(), oo.data_ptr(), oc.data_ptr()]
    pack = _lib.lib().gpk_pack_batch
    for m in (1 << 31, (1 << 31) + 5, 1 << 40):
        assert pack(ctypes.byref(b), good[0], m, good[2], good[3], good[4], None) == _lib.GPK_EINVAL, m
    for k in (0, 2, 3, 4):
        a = list(good)
        a[k] = None
        assert pack(ctypes.byref(b), *a, None) == _lib.GPK_EINVAL, k
    assert pack(None, *good, None) == _lib.GPK_EINVAL
    for k in range(3):  # the batch's own arrays
        f = [d.data_ptr(), o.data_ptr(), c.data_ptr()]
        f[k] = None
        assert pack(ctypes.byref(_lib.Batch(f[0], f[1], f[2], 2, d.numel())), *good, None) == _lib.GPK_EINVAL, k
    assert pack(ctypes.byref(b), None, 0, None, None, None, None) == _lib.GPK_OK
    assert pack(ctypes.byref(b), *good, None) == _lib.GPK_OK
    torch.cuda.synchronize()
    assert bytes(od[:7].cpu().numpy()) == b"abcabc\x00"  # order [0, 0] of the call above


def test_exchange_over_rccl_single_rank(gpu_ctx):
    import torch
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        d, o, c = synth.device_batch(6, 0, 20000)
        dest = torch.zeros(20000, dtype=torch.int64, device="cuda")
        dest[::5] = -1  # dropped
        rd, ro, rc, src, idx = shard.exchange_packets(d, o, c, dest, 1)
        torch.cuda.synchronize()
        keep = np.nonzero(dest.cpu().numpy() >= 0)[0]
        assert np.array_equal(idx.cpu().numpy(), keep) and np.all(src.cpu().numpy() == 0)
        hd, ho, hc = synth.host_batch(6, 0, 20000)
        rdn, ron, rcn = rd.cpu().numpy(), ro.cpu().numpy(), rc.cpu().numpy()
        for j in range(0, len(keep), 17):
            i = keep[j]
            assert bytes(rdn[ron[j]:ron[j] + rcn[j]]) == bytes(hd[ho[i]:ho[i] + hc[i]])
    finally:
        dist.destroy_process_group()
