"""gpk_decode_batch_narrow_compact (include/gpk.h): the narrow decode whose
widened packets' full records go to a compact sharded list (gpk_wide_list)
instead of the 16-byte-per-packet side array.

The reference of every comparison is gpk_decode_batch_narrow on the same batch
(pinned to the oracle by test_narrow_gpu.py) together with the CPU oracle's
narrow form. "Equality" (check_equal): records8, err_args and flows bit-equal
to the reference; the collected list is exactly {(i, wide[i]) : ST8_WIDE set};
total == the number of WIDE records; and the oracle agrees on all of it.

Cases: a hand-laid 600-packet batch whose waves are full / empty / widened only
at lane 0 / only at lane 63 / alternating / a partial last wave, with 1, 2 and
64 shards; overflow (a shard smaller than its share: nothing outside the
segment, every stored entry right, the count still whole) with canaries around
the arrays, and a count-only list; reuse of a list without clearing; the
golden packets under every parser; 40 000 fuzzed packets at two alignments; the
synthetic C4 and C2 mixes; n = 0 and n = 1; argument errors."""
import ctypes
import functools
import struct
import zlib

import numpy as np
import pytest

import pktutil
from configs import CONFIGS, device_parser, oracle_parser
from test_gpu_parity import golden_packets
from test_narrow_gpu import _ip4, _udp_ok, narrow_device

pytestmark = pytest.mark.gpu

CANARY = 0xC5


def _dev_batch(data, off, cap):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(data)).cuda(),
            torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(cap).view(np.int32)).cuda())


def _outputs(n):
    """records8 / err_args / flows filled as test_narrow_gpu.narrow_device fills them."""
    import torch
    return (torch.full((max(n, 1) * 8,), 0xAB, dtype=torch.uint8, device="cuda"),
            torch.zeros(max(2 * n, 1), dtype=torch.int32, device="cuda"),
            torch.zeros(max(3 * n, 1), dtype=torch.int64, device="cuda"))


def _host(rec8, err, fl, n):
    from gopacket_amd import _lib
    return dict(records8=rec8.cpu().numpy()[:8 * n].view(_lib.RECORD8_DTYPE),
                err_args=err.cpu().numpy()[:2 * n].view(np.uint32), flows=fl.cpu().numpy()[:3 * n].view(np.uint64))


def compact_device(ctx, cfg, data, off, cap, nshards, shard_cap=None, wl=None):
    """The batch through Context.decode_device_narrow_compact; shard_cap None = the never-overflow capacity."""
    import torch
    from gopacket_amd import engine
    n = len(off)
    d, o, c = _dev_batch(data, off, cap)
    rec8, err, fl = _outputs(n)
    if wl is None:
        wl = engine.WideList(nshards, engine.wide_shard_cap(n, nshards) if shard_cap is None else shard_cap)
    ctx.decode_device_narrow_compact(device_parser(cfg), d, o, c, rec8, wl, err, fl)
    torch.cuda.synchronize()
    got = _host(rec8, err, fl, n)
    got["index"], got["wide"], got["total"] = wl.collect()
    return got


_REFERENCE = {}


def reference(ctx, cfg_name, batch, key):
    """gpk_decode_batch_narrow of the batch, itself checked against the CPU oracle's narrow form; computed
    once per (parser, batch name) and shared by the tests that need it."""
    if (cfg_name, key) not in _REFERENCE:
        cfg = CONFIGS[cfg_name]
        ref = narrow_device(ctx, cfg, *batch)
        orc = oracle_parser(cfg).decode_narrow(*batch, nthreads=8)
        for k in ("records8", "wide", "err_args", "flows"):
            assert ref[k].tobytes() == orc[k].tobytes(), "reference %s differs from the oracle" % k
        _REFERENCE[(cfg_name, key)] = ref
    return _REFERENCE[(cfg_name, key)]


def check_equal(got, ref, what):
    from gopacket_amd import _lib
    for k in ("records8", "err_args", "flows"):
        assert got[k].tobytes() == ref[k].tobytes(), "%s: %s differs from gpk_decode_batch_narrow" % (what, k)
    w = np.nonzero(ref["records8"]["status"] & _lib.ST8_WIDE)[0]
    assert got["total"] == len(w), "%s: total %d, %d WIDE records" % (what, got["total"], len(w))
    assert np.array_equal(got["index"], w.astype(np.uint32)), "%s: list indices" % what
    assert got["wide"].tobytes() == ref["wide"][w].tobytes(), "%s: list records" % what
    return w


# ---- the edge batch: every shape of a wave's ballot ---------------------------

def _edge_batch():
    """600 packets; W = a UDP checksum of 0 (Valid, Correct != Actual: widened), N = a right one."""
    mac = b"\x02" * 12
    udp0 = struct.pack(">HHHH", 40000, 40001, 12, 0) + b"abcd"
    W = mac + b"\x08\x00" + _ip4(17, udp0)
    N = mac + b"\x08\x00" + _ip4(17, _udp_ok(b"abcd"))
    wide = set(range(0, 64))                 # a full wave
    #            64..127                       an empty wave
    wide.add(128)                            # lane 0 only
    wide.add(255)                            # lane 63 only
    wide.update(range(256, 320, 2))          # alternating
    #            320..575                      four empty waves
    wide.update((576, 599))                  # the last wave: 24 active lanes, its first and last
    pkts = [W if i in wide else N for i in range(600)]
    return pktutil.pack(pkts), np.array(sorted(wide))


@functools.lru_cache(maxsize=None)
def edge_batch():
    return _edge_batch()


def test_edge_batch_is_what_it_says():
    """CPU oracle: exactly the 100 intended packets are WIDE: 66 in block 0, 32 in block 1, 2 in block 2."""
    from gopacket_amd import _lib
    (data, off, cap), wide = edge_batch()
    orc = oracle_parser(CONFIGS["statsassembly"]).decode_narrow(data, off, cap)
    w = np.nonzero(orc["records8"]["status"] & _lib.ST8_WIDE)[0]
    assert np.array_equal(w, wide) and len(w) == 100
    assert [int(((w >> 8) == b).sum()) for b in range(3)] == [66, 32, 2]


@pytest.mark.parametrize("nshards", [1, 2, 64])
def test_edge_batch(gpu_ctx, nshards):
    batch, wide = edge_batch()
    ref = reference(gpu_ctx, "statsassembly", batch, "edge")
    got = compact_device(gpu_ctx, CONFIGS["statsassembly"], *batch, nshards)
    w = check_equal(got, ref, "edge/%d shards" % nshards)
    assert np.array_equal(w, wide)


# ---- overflow -----------------------------------------------------------------

def _run_raw(ctx, cfg, batch, nshards, shard_cap, with_arrays=True):
    """The C call on hand-laid arrays: 64 canary entries before and after index and records (one buffer each,
    the list inside it), every byte of the list itself canary too. Returns the host copies and the outputs."""
    import torch
    from gopacket_amd import _lib
    n = len(batch[1])
    d, o, c = _dev_batch(*batch)
    rec8, err, fl = _outputs(n)
    cap_entries = nshards * shard_cap
    idx = torch.full(((cap_entries + 128) * 4,), CANARY, dtype=torch.uint8, device="cuda")
    rec = torch.full(((cap_entries + 128) * 16,), CANARY, dtype=torch.uint8, device="cuda")
    cnt = torch.full((nshards * _lib.WIDE_COUNT_STRIDE,), 0x7777, dtype=torch.int32, device="cuda")
    wl = _lib.WideList(idx.data_ptr() + 64 * 4 if with_arrays else None, rec.data_ptr() + 64 * 16 if with_arrays else None,
                       cnt.data_ptr(), nshards, shard_cap)
    b = _lib.Batch(d.data_ptr(), o.data_ptr(), c.data_ptr(), n, d.numel())
    r = _lib.Results8(rec8.data_ptr(), None, err.data_ptr(), fl.data_ptr())
    p = device_parser(cfg)
    rc = _lib.lib().gpk_decode_batch_narrow_compact(ctx.h, p.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(wl), None)
    torch.cuda.synchronize()
    assert rc == 0
    return (idx.cpu().numpy().view(np.uint32), rec.cpu().numpy().view(_lib.RECORD_DTYPE),
            cnt.cpu().numpy().view(np.uint32), _host(rec8, err, fl, n))


def _is_canary(a):
    return bool(np.all(a.view(np.uint8) == CANARY))


@pytest.mark.parametrize("nshards,counts", [(2, [68, 32]), (1, [100])])
def test_overflow_is_contained(gpu_ctx, nshards, counts):
    """shard_cap 40. Two shards: shard 0 (blocks 0 and 2) draws 68 slots and stores 40, shard 1 (block 1) stores
    all its 32. One shard: 100 slots drawn, 40 stored. The segments are contiguous by the ABI, so what lies
    "after" shard 0 is shard 1's segment (checked entry by entry) and what lies after the last shard and before
    the first is canary; so is the unused tail of a shard that did not fill up."""
    from gopacket_amd import _lib
    batch, wide = edge_batch()
    ref = reference(gpu_ctx, "statsassembly", batch, "edge")
    idx, rec, cnt, out = _run_raw(gpu_ctx, CONFIGS["statsassembly"], batch, nshards, 40)
    for k in ("records8", "err_args", "flows"):
        assert out[k].tobytes() == ref[k].tobytes(), k
    assert [int(cnt[s * _lib.WIDE_COUNT_STRIDE]) for s in range(nshards)] == counts
    for s in range(nshards):
        stored = min(counts[s], 40)
        lo = 64 + s * 40
        members = wide[((wide >> 8) & (nshards - 1)) == s]
        got_i = idx[lo:lo + stored]
        assert len(set(got_i.tolist())) == stored and set(got_i.tolist()) <= set(members.tolist()), "shard %d" % s
        assert rec[lo:lo + stored].tobytes() == ref["wide"][got_i].tobytes(), "shard %d records" % s
        assert _is_canary(idx[lo + stored:lo + 40]) and _is_canary(rec[lo + stored:lo + 40]), "shard %d tail" % s
    assert _is_canary(idx[:64]) and _is_canary(rec[:64]), "before the list"
    assert _is_canary(idx[64 + nshards * 40:]) and _is_canary(rec[64 + nshards * 40:]), "after the list"


def test_count_only_list(gpu_ctx):
    """shard_cap 0 with NULL index and records: nothing stored, the counters still say 100."""
    from gopacket_amd import _lib
    batch, wide = edge_batch()
    ref = reference(gpu_ctx, "statsassembly", batch, "edge")
    idx, rec, cnt, out = _run_raw(gpu_ctx, CONFIGS["statsassembly"], batch, 2, 0, with_arrays=False)
    assert [int(cnt[0]), int(cnt[_lib.WIDE_COUNT_STRIDE])] == [68, 32]
    assert _is_canary(idx) and _is_canary(rec)
    for k in ("records8", "err_args", "flows"):
        assert out[k].tobytes() == ref[k].tobytes(), k


def test_reuse_without_clearing(gpu_ctx):
    """One list for the edge batch, then, uncleared, for 200 all-narrow packets: the library reset the counters."""
    from gopacket_amd import engine
    batch, wide = edge_batch()
    cfg = CONFIGS["statsassembly"]
    wl = engine.WideList(2, engine.wide_shard_cap(600, 2))
    got = compact_device(gpu_ctx, cfg, *batch, 2, wl=wl)
    check_equal(got, reference(gpu_ctx, "statsassembly", batch, "edge"), "first use")
    assert got["total"] == 100
    mac = b"\x02" * 12
    narrow = pktutil.pack([mac + b"\x08\x00" + _ip4(17, _udp_ok(bytes([i]) * (i % 37))) for i in range(200)])
    got = compact_device(gpu_ctx, cfg, *narrow, 2, wl=wl)
    check_equal(got, reference(gpu_ctx, "statsassembly", narrow, "narrow200"), "second use")
    assert got["total"] == 0 and len(got["index"]) == 0
    assert not wl.counts.cpu().numpy().any()


# ---- golden, fuzz, synthetic ----------------------------------------------------

@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_golden(gpu_ctx, cfg_name):
    batch = pktutil.pack(golden_packets())
    ref = reference(gpu_ctx, cfg_name, batch, "golden")
    check_equal(compact_device(gpu_ctx, CONFIGS[cfg_name], *batch, 64), ref, cfg_name)


@pytest.mark.parametrize("cfg_name", ["statsassembly", "eth_ip4_udp_payload"])
@pytest.mark.parametrize("align", [1, 16])
def test_fuzz(gpu_ctx, cfg_name, align):
    """40 000 fuzzed packets (157 blocks): 64 shards of 768 entries, the never-overflow capacity."""
    from gopacket_amd import engine
    packets = pktutil.fuzz_packets(zlib.crc32(cfg_name.encode()) % 1000 + 7 * align, 40000)
    batch = pktutil.pack(packets, align=align, pad=align // 2)
    assert engine.wide_shard_cap(40000, 64) == 768
    ref = reference(gpu_ctx, cfg_name, batch, "fuzz%d" % align)
    w = check_equal(compact_device(gpu_ctx, CONFIGS[cfg_name], *batch, 64, 768), ref, "%s/%d" % (cfg_name, align))
    assert 0 < len(w) < 40000


@pytest.mark.parametrize("synth_cfg,cfg_name", [(4, "statsassembly"), (2, "eth_ip4_udp_payload")])
def test_synthetic(gpu_ctx, synth_cfg, cfg_name):
    from gopacket_amd import synth
    batch = synth.host_batch(synth_cfg, 424242, 100000)
    ref = reference(gpu_ctx, cfg_name, batch, "synth%d" % synth_cfg)
    got = compact_device(gpu_ctx, CONFIGS[cfg_name], *batch, 64)
    check_equal(got, ref, "synth%d" % synth_cfg)
    assert 0 < got["total"] < 100000


# ---- degenerate sizes and arguments ---------------------------------------------

def _empty_batch():
    return np.zeros(16, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32)


def test_empty_batch(gpu_ctx):
    """n = 0: OK, and the counters (left non-zero by the caller) are all 0 afterwards."""
    from gopacket_amd import engine
    wl = engine.WideList(4, 8)
    wl.counts.fill_(9)
    got = compact_device(gpu_ctx, CONFIGS["statsassembly"], *_empty_batch(), 4, wl=wl)
    assert got["total"] == 0 and len(got["index"]) == 0 and len(got["records8"]) == 0
    assert not wl.counts.cpu().numpy().any()


def test_one_widened_packet(gpu_ctx):
    (data, off, cap), _ = edge_batch()
    batch = pktutil.pack([bytes(data[int(off[0]):int(off[0]) + int(cap[0])])])
    ref = reference(gpu_ctx, "statsassembly", batch, "one")
    got = compact_device(gpu_ctx, CONFIGS["statsassembly"], *batch, 64)
    check_equal(got, ref, "n = 1")
    assert got["total"] == 1 and list(got["index"]) == [0]


def test_argument_errors(gpu_ctx):
    """On an n = 0 batch, so that a missing check could launch nothing: each is GPK_EINVAL."""
    import torch
    from gopacket_amd import _lib
    d, o, c = _dev_batch(*_empty_batch())
    rec8, err, fl = _outputs(0)
    idx = torch.zeros(512 * 4, dtype=torch.int32, device="cuda")
    rec = torch.zeros(512 * 4 * 16 + 16, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(512 * _lib.WIDE_COUNT_STRIDE, dtype=torch.int32, device="cuda")
    p = device_parser(CONFIGS["statsassembly"])
    b = _lib.Batch(d.data_ptr(), o.data_ptr(), c.data_ptr(), 0, d.numel())
    r = _lib.Results8(rec8.data_ptr(), None, err.data_ptr(), fl.data_ptr())

    def call(index, records, counts, nshards, shard_cap):
        wl = _lib.WideList(index, records, counts, nshards, shard_cap)
        return _lib.lib().gpk_decode_batch_narrow_compact(gpu_ctx.h, p.h, ctypes.byref(b), ctypes.byref(r),
                                                          ctypes.byref(wl), None)
    I, R, C = idx.data_ptr(), rec.data_ptr(), cnt.data_ptr()
    assert R % 16 == 0
    assert call(I, R, C, 4, 4) == _lib.GPK_OK  # the well-formed call, for contrast
    assert call(I, R, C, 3, 4) == _lib.GPK_EINVAL
    assert call(I, R, C, 512, 4) == _lib.GPK_EINVAL
    assert call(I, R, C, 0, 4) == _lib.GPK_EINVAL
    assert call(I, R, None, 4, 4) == _lib.GPK_EINVAL
    assert call(None, R, C, 4, 4) == _lib.GPK_EINVAL
    assert call(I, None, C, 4, 4) == _lib.GPK_EINVAL
    assert call(I, R + 8, C, 4, 4) == _lib.GPK_EINVAL
    assert call(I, R, C, 256, 2**24) == _lib.GPK_EINVAL  # nshards * shard_cap = 2^32
    torch.cuda.synchronize()
