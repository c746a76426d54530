"""Timestamped fragment sequences for the timed reassembly tests
(tests/defrag_time_model.py, gpk_defrag_batch_timed, gpk_defrag6_batch_timed):
the inputs the CPU tests check the model's conditions on and the GPU tests run
on the device, so that a GPU test cannot pass vacuously."""
import functools

import numpy as np

import defrag6cases as D6
import defrag_time_model as TM
import defragcases as D4
import flowcases
import pktutil
from configs import oracle_parser

CFG4 = flowcases.DEFRAG_PARSER
CFG6 = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"])
T0 = 1700000000 * 10**9  # an ordinary capture time in ns
OLD, EDGE, YOUNG = 10, 50, 100


def ts(k):
    """k milliseconds after T0"""
    return T0 + k * 10**6


def decode(packets, cfg):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(cfg).decode(data, off, cap, layouts=True)
    return res["records"], res["layouts"]


def model4(packets, seen, ops=()):
    rec, lay = decode(packets, CFG4)
    return TM.run4(packets, rec, lay, seen, ops)


def model6(packets, seen, ops=(), carry=0):
    rec, lay = decode(packets, CFG6)
    return TM.run6(packets, rec, lay, seen, ops, carry=carry)


def conditions4():
    """-> (packets, seen, t, pending expected by hand, (keys, packets) discarded by hand).
    DiscardOlderThan(ts(EDGE)) after the batch."""
    f, b = D4.frag, lambda c, n: bytes([c]) * n
    rows = [
        (f(10, 0, 1, b(0x61, 16)), OLD),            # 0  A: restamped by 5, kept
        (f(11, 0, 1, b(0x62, 16)), OLD),            # 1  B: two old fragments, discarded
        (f(11, 2, 1, b(0x62, 16)), OLD + 1),        # 2
        (f(12, 0, 1, b(0x63, 16)), OLD),            # 3  C: its young call is an ignored duplicate, discarded
        (f(12, 0, 1, b(0x63, 16)), YOUNG),          # 4     (never pending)
        (f(10, 2, 1, b(0x61, 16)), YOUNG),          # 5  A's late fragment
        (f(13, 0, 1, b(0x64, 64)), OLD),            # 6  D: restamped by a counted, not listed fragment, kept
        (f(13, 4, 1, b(0x64, 16)), YOUNG),          # 7
        (f(14, 0, 1, b(0x65, 16)), EDGE),           # 8  E: LastSeen == t is not Before(t), kept
        (f(15, 0, 1, b(0x66, 16)), EDGE - 1),       # 9  F: one millisecond older, discarded
        (f(16, 0, 1, b(0x67, 16)), OLD),            # 10 G: restamped by a fragment whose build fails (hole), kept
        (f(16, 1, 1, b(0x67, 16)), OLD),            # 11
        (f(16, 4, 0, b(0x67, 8)), YOUNG),           # 12
        (f(17, 0, 1, b(0x68, 16)), OLD),            # 13 H: its young call fails the security checks, discarded
        (f(17, 2, 1, b(0x68, 4)), YOUNG),           # 14    (fragment too small: never reaches insert)
        (f(18, 0, 1, b(0x69, 8)), OLD),             # 15 I: completes while old, then starts again young, kept
        (f(18, 1, 0, b(0x69, 5)), OLD + 1),         # 16
        (f(18, 0, 1, b(0x69, 8)), YOUNG),           # 17
        (f(19, 0, 1, b(0x6A, 8)), OLD),             # 18 J: completes while old: no key left, nothing to discard
        (f(19, 1, 0, b(0x6A, 5)), OLD + 1),         # 19
        (b"\x00" * 11, YOUNG),                      # 20 no key
    ]
    return ([r[0] for r in rows], [ts(r[1]) for r in rows], ts(EDGE), [0, 5, 6, 7, 8, 10, 11, 12, 17], (4, 5))


def conditions6():
    """As conditions4, for ip6defrag: every call on a key stamps it."""
    f, p = D6.frag6, [bytes([0x41 + k]) * 8 for k in range(4)]
    rows = [
        (f(20, 0, 1, p[0]), OLD),        # 0  A: its young call is an ignored duplicate, which stamps: kept
        (f(20, 0, 1, p[1]), YOUNG),      # 1     (not listed)
        (f(21, 0, 1, p[0]), OLD),        # 2  B: lone and old, discarded
        (f(22, 1, 1, p[0]), EDGE),       # 3  C: time == t is not Before(t), kept
        (f(23, 1, 1, p[0]), EDGE - 1),   # 4  D: one millisecond older, discarded
        (f(24, 0, 1, p[0]), OLD),        # 5  E: the call that returns its datagram stamps, kept (nothing is removed)
        (f(24, 1, 0, p[1]), YOUNG),      # 6
        (f(25, 0, 1, p[0]), OLD),        # 7  F: complete and old: its datagram is returned, then it is discarded
        (f(25, 1, 0, p[1]), OLD + 1),    # 8
        (f(26, 2, 0, p[2]), OLD),        # 9  G: a young fragment becomes the head and is the entry stamped, kept
        (f(26, 1, 1, p[1]), YOUNG),      # 10
        (b"\x00" * 11, YOUNG),           # 11 no key
    ]
    return ([r[0] for r in rows], [ts(r[1]) for r in rows], ts(EDGE), [0, 3, 5, 6, 9, 10], (3, 4))


WINDOW = 15  # the streams discard what has been quiet for 15 ms, one packet a millisecond


@functools.lru_cache(maxsize=None)
def stream4():
    """-> (packets, seen, ops): about 60 fragments of interleaved datagrams with
    reordering, duplicates, drops and corrupted fields, one a millisecond, and
    three DiscardOlderThan(now - 15 ms) at fixed positions."""
    pk = D4.random_traffic(31, 14, lo=500, hi=1400, per=256, window=10, dup=0.1, drop=0.12, corrupt=0.05)
    # two lone fragments that age out, at positions 2 and 30
    pk = pk[:2] + [D4.frag(701, 0, 1, b"o" * 16)] + pk[2:29] + [D4.frag(700, 0, 1, b"q" * 16)] + pk[29:]
    seen = [ts(i) for i in range(len(pk))]
    ops = [(p, ts(p - WINDOW)) for p in (20, 41, len(pk))]
    return pk, seen, ops


@functools.lru_cache(maxsize=None)
def stream6():
    """As stream4 for IPv6, plus key 900 whose last call before a discard is an
    ignored duplicate: only that call's stamp keeps it."""
    pk = D6.random_traffic(32, 14, lo=500, hi=1400, per=256, window=10, dup=0.1, drop=0.12, vlan_every=3)
    lone = D6.frag6(900, 0, 1, b"r" * 8)
    # a lone fragment that ages out at position 2, key 900 at positions 12 and 37
    pk = pk[:2] + [D6.frag6(901, 1, 1, b"o" * 8)] + pk[2:11] + [lone] + pk[11:35] + [lone] + pk[35:]
    seen = [ts(i) for i in range(len(pk))]
    ops = [(p, ts(p - WINDOW)) for p in (20, 41, len(pk))]
    return pk, seen, ops


def segments(n, ops, cut):
    """The packet ranges between the stream's discards and one batch cut:
    [(lo, hi, [t, ...] to discard after it)], covering 0..n in order."""
    assert all(0 < p <= n for p, _ in ops)
    marks = sorted({0, n, cut} | {p for p, _ in ops})
    return [(lo, hi, [t for p, t in ops if p == hi]) for lo, hi in zip(marks, marks[1:])]


def as_int64(seen):
    return np.array(seen, dtype=np.int64)
