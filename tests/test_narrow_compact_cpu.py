"""gpk_wide_collect (include/gpk.h): the host-side merge of a copied-back
gpk_wide_list, on hand-made arrays: no GPU call. Shards with 0, some, exactly
shard_cap and more than shard_cap (overflowed) widened packets, entries
shuffled inside each shard and poison in every unused slot; and the argument
errors."""
import ctypes

import numpy as np
import pytest

from gopacket_amd import _lib, engine

POISON = 0xDEADBEEF


def _list(nshards, cap, counts, seed=5):
    """A host list whose shard s holds min(counts[s], cap) entries: packet
    indices of the blocks that map to shard s, shuffled, each with a record
    derived from its index; poison everywhere else."""
    rng = np.random.default_rng(seed)
    index = np.full(nshards * cap, POISON, np.uint32)
    records = np.zeros(nshards * cap, _lib.RECORD_DTYPE)
    records.view(np.uint8)[:] = 0xEE
    cnt = np.full(nshards * _lib.WIDE_COUNT_STRIDE, POISON, np.uint32)
    want = []
    for s, c in enumerate(counts):
        cnt[s * _lib.WIDE_COUNT_STRIDE] = c
        # packets of blocks s, s + nshards, ...: 256 * block + lane
        pool = np.array([256 * (s + nshards * b) + l for b in range(2) for l in range(0, 256, 37)], np.uint32)
        take = rng.permutation(pool)[:min(c, cap)]
        for k, i in enumerate(take):
            index[s * cap + k] = i
            records[s * cap + k] = (int(i) * 0x9E3779B97F4A7C15 % 2**64, int(i) ^ 0x5A5A, int(i) % 65536, 65535 - int(i) % 65536)
            want.append(int(i))
    return index, records, cnt, sorted(want)


def test_wide_collect_random_fill():
    index, records, cnt, want = _list(4, 8, [0, 3, 8, 11])
    idx, rec, total = engine.wide_collect(index, records, cnt, 4, 8)
    assert len(idx) == 19 and total == 22  # the last shard overflowed: 8 of its 11 are stored
    assert list(idx) == want and POISON not in idx
    assert np.all(np.diff(idx.astype(np.int64)) > 0)
    for i, r in zip(idx, rec):
        i = int(i)
        assert (int(r["layers"]), int(r["status"]), int(r["ip4_csum"]), int(r["l4_csum"])) == (
            i * 0x9E3779B97F4A7C15 % 2**64, i ^ 0x5A5A, i % 65536, 65535 - i % 65536)


def test_wide_collect_counts_only_and_empty():
    cnt = np.zeros(2 * _lib.WIDE_COUNT_STRIDE, np.uint32)
    cnt[0], cnt[_lib.WIDE_COUNT_STRIDE] = 7, 5
    idx, rec, total = engine.wide_collect(np.zeros(0, np.uint32), np.zeros(0, _lib.RECORD_DTYPE), cnt, 2, 0)
    assert len(idx) == 0 and len(rec) == 0 and total == 12
    index, records, cnt, _ = _list(1, 4, [0])
    idx, rec, total = engine.wide_collect(index, records, cnt, 1, 4)
    assert len(idx) == 0 and total == 0


@pytest.mark.parametrize("nshards", [0, 3, 512])
def test_wide_collect_bad_nshards(nshards):
    index, records, cnt, _ = _list(4, 8, [1, 1, 1, 1])
    cnt = np.resize(cnt, 512 * _lib.WIDE_COUNT_STRIDE)
    out_i, out_r = np.zeros(4096, np.uint32), np.zeros(4096, _lib.RECORD_DTYPE)
    wl = _lib.WideList(index.ctypes.data, records.ctypes.data, cnt.ctypes.data, nshards, 8)
    stored, total = ctypes.c_uint64(), ctypes.c_uint64()
    rc = _lib.lib().gpk_wide_collect(ctypes.byref(wl), out_i.ctypes.data, out_r.ctypes.data, ctypes.byref(stored),
                                     ctypes.byref(total))
    assert rc == _lib.GPK_EINVAL


def test_wide_collect_null_arguments():
    index, records, cnt, _ = _list(4, 8, [1, 1, 1, 1])
    out_i, out_r = np.zeros(32, np.uint32), np.zeros(32, _lib.RECORD_DTYPE)
    stored, total = ctypes.c_uint64(), ctypes.c_uint64()
    L = _lib.lib()
    for wl in (_lib.WideList(index.ctypes.data, records.ctypes.data, None, 4, 8),
               _lib.WideList(None, records.ctypes.data, cnt.ctypes.data, 4, 8),
               _lib.WideList(index.ctypes.data, None, cnt.ctypes.data, 4, 8)):
        assert L.gpk_wide_collect(ctypes.byref(wl), out_i.ctypes.data, out_r.ctypes.data, ctypes.byref(stored),
                                  ctypes.byref(total)) == _lib.GPK_EINVAL
    wl = _lib.WideList(index.ctypes.data, records.ctypes.data, cnt.ctypes.data, 4, 8)
    assert L.gpk_wide_collect(ctypes.byref(wl), None, out_r.ctypes.data, ctypes.byref(stored),
                              ctypes.byref(total)) == _lib.GPK_EINVAL
    assert L.gpk_wide_collect(None, out_i.ctypes.data, out_r.ctypes.data, ctypes.byref(stored),
                              ctypes.byref(total)) == _lib.GPK_EINVAL


def test_never_overflow_capacity():
    # every 256-packet block of a shard all widened: ceil(ceil(n / 256) / nshards) * 256
    assert engine.wide_shard_cap(0, 64) == 0
    assert engine.wide_shard_cap(1, 64) == 256
    assert engine.wide_shard_cap(600, 2) == 512 and engine.wide_shard_cap(600, 1) == 768
    assert engine.wide_shard_cap(40000, 64) == 768  # 157 blocks over 64 shards
    assert engine.wide_shard_cap(64 * 2**20, 64) == 2**20
