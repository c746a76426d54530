"""A numpy restatement of the grouping key words and their 64-bit hash
(gopacket_amd/csrc/gpk_flows.hip key_kernel, gpk_kernels.hip derive_key), and
a finder of adversarial keys: different keys whose hashes share the table's
36-bit tag and home slot, and keys whose home slots lie in a chosen set.

The hash table of a Grouper(max_packets) has T = the smallest power of two
>= 2 * max_packets slots; a key's home slot is h & (T - 1), the slot word keeps
h >> 28 as the tag. Nothing found here is hard-coded: when the hash changes,
tests/test_flows_table_gpu.py::test_restatement_holds fails first and this
file is updated, and the finder then finds other keys.

Key words w[0..9] (little-endian dwords of the Flow bytes):
  CONNECTION  w0 = 1 | net << 8 | 4 << 16 (net 1 = IPv4, 2 = IPv6),
              w1.. = source address, w5.. = destination address,
              w9 = the four port bytes
  DEFRAG      w0 = 2 | 1 << 8, w1 = source, w5 = destination, w9 = Id
"""
import functools
import struct

import numpy as np

KEY_WORDS = 10
IDX_BITS = 28
_SEED = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def table_size(max_packets):
    t = 1
    while t < 2 * max_packets:
        t <<= 1
    return t


def hash_words(w):
    """w: uint32 array [..., 10] -> uint64 hashes [...]."""
    w = np.asarray(w, np.uint64)
    h = np.full(w.shape[:-1], _SEED, np.uint64)
    with np.errstate(over="ignore"):
        for k in range(KEY_WORDS):
            h = (h ^ w[..., k]) * _M1
            h ^= h >> np.uint64(29)
        h = (h ^ (h >> np.uint64(30))) * _M1
        h = (h ^ (h >> np.uint64(27))) * _M2
        h ^= h >> np.uint64(31)
    return h


def _le32(b):
    return struct.unpack("<I", bytes(b))[0]


def key_words(key):
    """The ten key words of an oracle key (oracle/flows_oracle.py packet_key):
    ("conn", (net, src, dst), (4, sport, dport)) or ("frag", (1, src, dst), id)."""
    w = [0] * KEY_WORDS
    if key[0] == "conn":
        net, src, dst = key[1]
        w[0] = 1 | net << 8 | 4 << 16
        for k in range(len(src) // 4):
            w[1 + k] = _le32(src[4 * k:4 * k + 4])
            w[5 + k] = _le32(dst[4 * k:4 * k + 4])
        w[9] = _le32(key[2][1] + key[2][2])
    elif key[0] == "frag":
        _, src, dst = key[1]
        w[0] = 2 | 1 << 8
        w[1], w[5], w[9] = _le32(src), _le32(dst), key[2]
    else:
        raise ValueError(key[0])
    return w


def key_hash(key):
    return int(hash_words(np.array(key_words(key), np.uint32)))


# ---------------------------------------------------------------------------
# candidates: index c -> a key's field values. DEFRAG varies the 16-bit Id and
# two source-address bytes, CONNECTION the source port and a source-address
# byte (up to 2^24 candidates each).

DST = (10, 200, 0, 2)
DPORT = 40000


def candidate(kind, c):
    """-> dict(src, dst, ident) for "frag", dict(src, dst, sport, dport) for "conn"."""
    c = int(c)
    lo, hi = c & 0xFFFF, c >> 16
    if kind == "frag":
        return dict(src=(10, 1, hi & 255, 1 + (hi >> 8)), dst=DST, ident=lo)
    return dict(src=(10, 2, 0, hi & 255), dst=DST, sport=lo, dport=DPORT)


def candidate_words(kind, count):
    c = np.arange(count, dtype=np.uint64)
    lo, hi = c & np.uint64(0xFFFF), c >> np.uint64(16)
    w = np.zeros((count, KEY_WORDS), np.uint32)
    dst = _le32(bytes(DST))
    w[:, 5] = dst
    if kind == "frag":
        assert count <= 1 << 24
        w[:, 0] = 2 | 1 << 8
        b2, b3 = hi & np.uint64(255), np.uint64(1) + (hi >> np.uint64(8))
        w[:, 1] = 10 | 1 << 8 | b2 << np.uint64(16) | b3 << np.uint64(24)
        w[:, 9] = lo
    else:
        assert count <= 1 << 24
        w[:, 0] = 1 | 1 << 8 | 4 << 16
        w[:, 1] = 10 | 2 << 8 | (hi & np.uint64(255)) << np.uint64(24)
        # port bytes big-endian in the packet, read as a little-endian dword
        sp = (lo >> np.uint64(8)) | (lo & np.uint64(255)) << np.uint64(8)
        w[:, 9] = sp | np.uint64((DPORT >> 8) | (DPORT & 255) << 8) << np.uint64(16)
    return w


def candidate_key(kind, c):
    """The oracle's key tuple of candidate c."""
    f = candidate(kind, c)
    if kind == "frag":
        return ("frag", (1, bytes(f["src"]), bytes(f["dst"])), f["ident"])
    return ("conn", (1, bytes(f["src"]), bytes(f["dst"])),
            (4, struct.pack(">H", f["sport"]), struct.pack(">H", f["dport"])))


START, LIMIT = 1 << 22, 1 << 24


@functools.lru_cache(maxsize=2)
def candidate_hashes(kind, count):
    h = hash_words(candidate_words(kind, count))
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def find_pairs(kind, tsize, want=2):
    """Pairs (a, b) of candidate indices, a < b, with different keys, equal
    tag (h >> 28) and equal home slot (h & (tsize - 1)). Enumerates 2^22
    candidates, more (up to 2^24) while fewer than `want` pairs are found.
    -> (pairs, stats) with stats = dict(candidates, equal_tag, usable)."""
    count = START
    while True:
        h = candidate_hashes(kind, count)
        tag = h >> np.uint64(IDX_BITS)
        order = np.argsort(tag, kind="stable")
        ts = tag[order]
        eq = np.nonzero(ts[1:] == ts[:-1])[0]
        pairs = []
        for j in eq:
            a, b = sorted((int(order[j]), int(order[j + 1])))
            if h[a] == h[b]:
                continue  # an equal hash says nothing about same_key's tag path; not expected at all
            if (int(h[a]) ^ int(h[b])) & (tsize - 1) == 0:
                pairs.append((a, b))
        stats = dict(candidates=count, equal_tag=len(eq), usable=len(pairs))
        if len(pairs) >= want or count >= LIMIT:
            break
        count <<= 1
    assert len(pairs) >= want, "grouphash.find_pairs(%s, T=%d): %r" % (kind, tsize, stats)
    for a, b in pairs:
        assert candidate_key(kind, a) != candidate_key(kind, b)
    return pairs, stats


@functools.lru_cache(maxsize=None)
def find_homed(kind, tsize, slots, want):
    """`want` candidate indices (ascending) whose home slot h & (tsize - 1) is
    in `slots`, spread evenly over the slots. -> (indices, stats)."""
    slots = sorted(set(int(s) for s in slots))  # `slots` is a tuple (the cache's key)
    count = START
    while True:
        h = candidate_hashes(kind, count)
        home = (h & np.uint64(tsize - 1)).astype(np.int64)
        per = -(-want // len(slots))
        got = [np.nonzero(home == s)[0][:per] for s in slots]
        idx = np.sort(np.concatenate(got))[:want] if all(len(g) >= per for g in got) else np.zeros(0, np.int64)
        stats = dict(candidates=count, per_slot=[int((home == s).sum()) for s in slots], chain=len(idx))
        if len(idx) >= want or count >= LIMIT:
            break
        count <<= 1
    assert len(idx) >= want, "grouphash.find_homed(%s, T=%d, %r): %r" % (kind, tsize, slots, stats)
    assert len(set(candidate_key(kind, c) for c in idx)) == len(idx)
    return [int(c) for c in idx], stats
