"""Timestamped TCP sequences for the timed reassembly tests
(tests/tcpasm_time_model.py, gpk_tcpasm_batch_timed): the inputs the CPU tests
check the model's conditions on and the GPU tests run on the device, so that a
GPU test cannot pass vacuously."""
import functools

import numpy as np

import flowcases
import pktutil
import tcpasm_model as M
import tcpasm_time_model as TM
import tcpasmcases as TC
from configs import oracle_parser

CFG = flowcases.DEFRAG_PARSER
T0 = 1700000000 * 10**9
OLD, EDGE, YOUNG = 10, 50, 100
S, F = TC.SYN, TC.FIN


def ts(k):
    """k milliseconds after T0"""
    return T0 + k * 10**6


def model(packets, seen, ops=(), **kw):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(CFG).decode(data, off, cap, layouts=True)
    return TM.run(packets, res["records"], res["layouts"], seen, ops, **kw)


def device_codes(ref):
    """The model's result with ("flush", op, round) written as the device writes
    it for a single batch: CALL_FLUSH | round."""
    def code(c):
        return M.CALL_FLUSH | c[2] if isinstance(c, tuple) else c
    for st in ref["streams"]:
        st["closed"] = code(st["closed"])
        for ch in st["chunks"]:
            ch["call"] = code(ch["call"])
    return ref


PEAKS = (0, 1, 63, 64, 65, 129, 130)


@functools.lru_cache(maxsize=None)
def last_seen_keys():
    """-> (packets, seen, expected lastSeen per key). One key per peak position:
    a SYN and 130 in-order segments (two and a bit steps of the 64-packet fast
    path), left open, every timestamp 1000 except the single largest at that
    position; then a key whose timestamps are shuffled (lastSeen is a maximum,
    not the last value) and one whose timestamps fall all the way."""
    rng = np.random.default_rng(61)
    pk, seen, want = [], [], []
    for q, peak in enumerate(PEAKS):
        segs = TC.stream_segments(rng, int(rng.integers(0, 2 ** 32)), [int(x) for x in rng.integers(1, 200, 130)],
                                  fin=False, sport=6000 + q)
        pk += segs
        seen += [ts(2000 + q) if j == peak else ts(1000) for j in range(len(segs))]
        want.append(ts(2000 + q))
    segs = TC.stream_segments(rng, 5, [int(x) for x in rng.integers(1, 200, 130)], fin=False, sport=6100)
    mixed = [ts(int(x)) for x in rng.permutation(len(segs))]
    pk += segs
    seen += mixed
    want.append(max(mixed))
    segs = TC.stream_segments(rng, 9, [int(x) for x in rng.integers(1, 200, 130)], fin=False, sport=6101)
    pk += segs
    seen += [ts(500 - j) for j in range(len(segs))]
    want.append(ts(500))
    return pk, seen, want


def boundary_keys():
    """-> (packets, seen, {name: stream number}). Every connection of the
    boundary tests, T = ts(EDGE); by hand, per name, what FlushWithOptions does:

      first==T      a queued page with Seen == T: not Before(T), untouched
      first==T-1    one nanosecond older: flushed (round 0, Skip 4), drained; lastSeen T-1 < T: CloseAll closes it
      drained==T    no pages, lastSeen == T: stays open in both modes
      drained==T-1  no pages, lastSeen == T-1: closed by CloseAll (mode 2) only
      nosyn         no SYN, so nextSeq is invalid: its old page goes out with Skip -1; lastSeen is young, stays open
      multipage     a 5000-byte segment queued behind a hole: three pages with one Seen, all out in round 0
      shield        a young first page in front of an older page: nothing happens
      fin           an old queued FIN behind a hole: round 0's chunk has End, the connection closes inside the loop
      comment       FlushWithOptions' own example (assembly.go:216-226): processed through 10, pages
                    [15,20) [20,25) [30,50); [15,20) is old: [15,25) goes out with Skip 5, [30,50) is young and stays
      comment-old   the same with [30,50) old as well: a second round, Skip 5
      young         everything young: untouched
    """
    T = ts(EDGE)
    rows, names = [], []

    def key(name, items):
        port = 7000 + len(names)
        names.append(name)
        rows.extend((TC.seg(seq, fl, pay, sport=port), when) for seq, fl, pay, when in items)

    key("first==T", [(100, S, b"", ts(OLD)), (105, 0, b"abc", T)])
    key("first==T-1", [(100, S, b"", ts(OLD)), (105, 0, b"abc", T - 1)])
    key("drained==T", [(100, S, b"", ts(OLD)), (101, 0, b"ab", T)])
    key("drained==T-1", [(100, S, b"", ts(OLD)), (101, 0, b"ab", T - 1)])
    key("nosyn", [(500, 0, b"wait", ts(OLD)), (600, 0, b"more", ts(YOUNG))])
    key("multipage", [(100, S, b"", ts(OLD)), (201, 0, bytes(range(256)) * 19 + b"x" * 136, ts(OLD + 1))])
    key("shield", [(100, S, b"", ts(OLD)), (300, 0, b"older, behind", ts(OLD)), (200, 0, b"young, first", ts(YOUNG))])
    key("fin", [(100, S, b"", ts(OLD)), (150, F, b"bye", ts(OLD + 2))])
    key("comment", [(4, S, b"hello", ts(OLD)), (15, 0, b"fffff", ts(OLD)), (20, 0, b"ggggg", ts(YOUNG)),
                    (30, 0, b"h" * 20, ts(YOUNG))])
    key("comment-old", [(4, S, b"hello", ts(OLD)), (15, 0, b"fffff", ts(OLD)), (20, 0, b"ggggg", ts(YOUNG)),
                        (30, 0, b"h" * 20, ts(OLD))])
    key("young", [(100, S, b"", ts(YOUNG)), (105, 0, b"abc", ts(YOUNG))])
    return [r[0] for r in rows], [r[1] for r in rows], {n: j for j, n in enumerate(names)}


@functools.lru_cache(maxsize=None)
def long_list():
    """-> (packets, seen, T): one key of 300 queued single-page segments with
    gaps between them (above the 256 list positions kept in LDS), the first 270
    old: 270 rounds of one page each, the head moving across position 256."""
    pk = [TC.seg(1000 + 10 * j, 0, bytes([j & 255]) * 5, sport=7500) for j in range(300)]
    seen = [ts(OLD) if j < 270 else ts(YOUNG) for j in range(300)]
    return pk, seen, ts(EDGE)


WINDOW = 20


@functools.lru_cache(maxsize=None)
def stream():
    """-> (packets, seen, ops): 150 packets of mixed traffic, one a millisecond,
    with FlushOlderThan(now - 20 ms) before positions 50 and 100, the second
    without CloseAll, and FlushOlderThan after the last one."""
    rng = np.random.default_rng(71)
    pk = TC.random_traffic(13, 24, lo=2, hi=7)[:141]
    kw = dict(sport=9)
    pk[20:20] = [TC.seg(100, S, **kw), TC.seg(2201, 0, TC.body(rng, 5000), **kw)]   # three pages waiting behind a hole
    pk[60:60] = [TC.seg(7, S, sport=10), TC.seg(8, 0, b"idle", sport=10)]            # drained, goes stale
    pk[70:70] = [TC.seg(300, 0, b"older", sport=11)]
    pk[95:95] = [TC.seg(200, 0, b"young first page", sport=11)]                      # shields the older page at 100
    pk[120:120] = [TC.seg(900, 0, b"late", sport=9), TC.seg(50, F, b"fin", sport=12), TC.seg(40, S, sport=12)]
    assert len(pk) == 150
    seen = [ts(i) for i in range(150)]
    ops = [(50, ts(50 - WINDOW), True), (100, ts(100 - WINDOW), False), (150, ts(150 - WINDOW), True)]
    return pk, seen, ops


def segments(n, ops, cut):
    """The packet ranges between the stream's flushes and one batch cut:
    [(lo, hi, [op number, ...] to run after it)], covering 0..n in order."""
    assert all(0 < o[0] <= n for o in ops)
    marks = sorted({0, n, cut} | {o[0] for o in ops})
    return [(lo, hi, [k for k, o in enumerate(ops) if o[0] == hi]) for lo, hi in zip(marks, marks[1:])]


def backwards_case():
    """-> (packets, seen). The one place the free list shows: connection X
    (port 1) closes with lastSeen 100; Y (port 2) is created next, so with the
    reference's LIFO free list it gets X's struct and starts from lastSeen 100,
    while its own packets are stamped 20 and 21: timestamps running backwards.
    FlushOlderThan(50) then finds Y drained: the device's rule (a fresh lastSeen:
    21 < 50) closes it, the reference's (100, not Before(50)) leaves it open."""
    pk = [TC.seg(10, S, sport=1), TC.seg(11, F, b"x", sport=1), TC.seg(10, S, sport=2), TC.seg(11, 0, b"y", sport=2)]
    return pk, [ts(99), ts(100), ts(20), ts(21)]


def as_int64(seen):
    return np.array(seen, dtype=np.int64)
