"""Packets for the TCP reassembly tests: real Ethernet/IP/TCP frames built from
layers.TCP{Seq, flags, Payload} values, the sequences of tcpassembly's own
tests (assembly_test.go) with their `want` lists, and random traffic."""
import struct

import numpy as np

import flowcases

FIN, SYN, RST, PSH, ACK = 1, 2, 4, 8, 16
A4, B4 = (1, 2, 3, 4), (5, 6, 7, 8)  # assembly_test.go:21-25
PAGE = 1900


def seg(seq, flags=0, payload=b"", src=A4, dst=B4, sport=1, dport=2, v6=False, vlan=None, pad=0):
    """flowcases.tcp_segment with a sequence number, and optionally a VLAN tag.
    ACK is added to a flagless segment so that it looks like traffic; the
    assembler reads SYN, FIN and RST only."""
    payload = bytes(payload)
    if v6 and len(src) == 4:
        src, dst = bytes(src) * 4, bytes(dst) * 4
    f = flowcases.tcp_segment(src, dst, sport, dport, flags or ACK, payload, v6=v6, pad=pad)
    l3 = 14
    hl = 40 if v6 else 20
    f = bytearray(f)
    struct.pack_into(">I", f, l3 + hl + 4, seq & 0xFFFFFFFF)
    if vlan is not None:
        f = f[:12] + b"\x81\x00" + struct.pack(">H", vlan) + f[12:]
    return bytes(f)


def R(b=b"", skip=0, start=False, end=False):
    return (bytes(b), skip, start, end)


D10 = bytes([1, 2, 3, 4, 5, 6, 7, 8, 9, 0])
BIG = bytes(PAGE * 3)

# name -> [(Seq, SYN, payload, want)]: assembly_test.go, MaxBufferedPagesPerConnection = 4 (:58)
REFERENCE = {
    "TestReorder": [  # :68-158
        (1001, 0, [1, 2, 3], []),
        (1004, 0, [2, 2, 3], []),
        (1010, 0, [4, 2, 3], []),
        (1007, 0, [3, 2, 3], [R([1, 2, 3], skip=-1), R([2, 2, 3]), R([3, 2, 3]), R([4, 2, 3])]),
        (1016, 0, [2, 2, 3], []),
        (1019, 0, [3, 2, 3], []),
        (1013, 0, [1, 2, 3], [R([1, 2, 3]), R([2, 2, 3]), R([3, 2, 3])]),
    ],
    "TestMaxPerSkip": [  # :160-228
        (1000, 1, [1, 2, 3], [R([1, 2, 3], start=True)]),
        (1007, 0, [3, 2, 3], []),
        (1010, 0, [4, 2, 3], []),
        (1013, 0, [5, 2, 3], []),
        (1016, 0, [6, 2, 3], [R([3, 2, 3], skip=3), R([4, 2, 3]), R([5, 2, 3]), R([6, 2, 3])]),
    ],
    "TestReorderFast": [  # :230-273
        (1000, 1, [1, 2, 3], [R([1, 2, 3], start=True)]),
        (1007, 0, [3, 2, 3], []),
        (1004, 0, [2, 2, 3], [R([2, 2, 3]), R([3, 2, 3])]),
    ],
    "TestOverlap": [  # :275-319
        (1000, 1, D10, [R(D10, start=True)]),
        (1007, 0, [7, 8, 9, 0, 1, 2, 3, 4, 5], [R([1, 2, 3, 4, 5])]),
        (1010, 0, [0, 1, 2, 3, 4, 5, 6, 7], [R([6, 7])]),
    ],
    "TestBufferedOverlap": [  # :321-363
        (1007, 0, [7, 8, 9, 0, 1, 2, 3, 4, 5], []),
        (1010, 0, [0, 1, 2, 3, 4, 5, 6, 7], []),
        (1000, 1, D10, [R(D10, start=True), R([1, 2, 3, 4, 5]), R([6, 7])]),
    ],
    "TestOverrun1": [  # :365-396
        (0xFFFFFFFF, 1, D10, [R(D10, start=True)]),
        (10, 0, [1, 2, 3, 4], [R([1, 2, 3, 4])]),
    ],
    "TestOverrun2": [  # :398-428
        (10, 0, [1, 2, 3, 4], []),
        (0xFFFFFFFF, 1, D10, [R(D10, start=True), R([1, 2, 3, 4])]),
    ],
    "TestCacheLargePacket": [  # :430-467
        (1001, 0, BIG, []),
        (1000, 1, b"", [R(b"", start=True), R(BIG[:PAGE]), R(BIG[PAGE:2 * PAGE]), R(BIG[2 * PAGE:])]),
    ],
}


def reference_packets(name):
    return [seg(s, SYN if syn else 0, bytes(p)) for s, syn, p, _ in REFERENCE[name]]


def body(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def stream_segments(rng, isn, sizes, syn=True, fin=True, **kw):
    """An in-order connection: SYN (no payload), data segments, FIN."""
    out, seq = [], isn
    if syn:
        out.append(seg(seq, SYN, **kw))
        seq += 1
    for n in sizes:
        out.append(seg(seq, 0, body(rng, n), **kw))
        seq += n
    if fin:
        out.append(seg(seq, FIN | ACK, **kw))
    return out


def random_traffic(seed, conns, lo=2, hi=14):
    """`conns` connections with interleaved keys: reordering, loss, duplication,
    overlap, multi-page segments, missing SYNs, data after FIN; IPv4, IPv6 and
    VLAN frames; ISNs near the wrap points."""
    rng = np.random.default_rng(seed)
    isns = [0, 2 ** 30 - 1, 2 ** 30, 3 * 2 ** 30, 3 * 2 ** 30 + 1, 2 ** 32 - 1, 2 ** 32 - 10]
    per = []
    for c in range(conns):
        kw = dict(src=(10, c >> 16 & 255, c >> 8 & 255, c & 255), dst=(10, 200, 0, 1 + c % 3), sport=1024 + c % 50000,
                  dport=80 + c % 7)
        m = c % 8
        if m == 5:
            kw["v6"] = True
        if m == 6:
            kw["vlan"] = 7
        isn = isns[c % len(isns)] if c % 3 == 0 else int(rng.integers(0, 2 ** 32))
        if c % 4 == 0:
            isn = (isns[c % len(isns)] - int(rng.integers(0, 3000))) % 2 ** 32
        k = int(rng.integers(lo, hi))
        sizes = [int(x) for x in rng.choice([1, 7, 100, 536, 1448, 1899, 1900, 1901, 4000], k)]
        segs = stream_segments(rng, isn, sizes, syn=c % 5 != 1, fin=c % 6 != 2, **kw)
        kind = c % 7
        if kind == 1 and len(segs) > 3:    # reordering
            j = int(rng.integers(1, len(segs) - 1))
            segs[j], segs[j + 1] = segs[j + 1], segs[j]
        elif kind == 2 and len(segs) > 3:  # loss
            del segs[int(rng.integers(1, len(segs) - 1))]
        elif kind == 3:                    # duplication
            j = int(rng.integers(0, len(segs)))
            segs.insert(min(len(segs), j + int(rng.integers(0, 3))), segs[j])
        elif kind == 4 and len(segs) > 2:  # overlap: a segment that starts inside its predecessor
            seq = isn + 1 + sizes[0] - min(sizes[0], 5)
            segs.insert(2, seg(seq, 0, body(rng, 40), **kw))
        elif kind == 5:                    # shuffled within a window
            segs = [segs[j] for j in sorted(range(len(segs)), key=lambda j: j + 3 * rng.random())]
        elif kind == 6:                    # data after FIN, and the other direction
            segs.append(seg(isn + 77, 0, body(rng, 9), **kw))
            kw2 = dict(kw, src=kw["dst"], dst=kw["src"], sport=kw["dport"], dport=kw["sport"])
            segs += stream_segments(rng, int(rng.integers(0, 2 ** 32)), sizes[:2], **kw2)
        per.append(segs)
    out, at = [], [0] * conns  # interleave: a few connections are live at a time
    live = list(range(min(conns, 24)))
    nxt = len(live)
    while live:
        c = live[int(rng.integers(0, len(live)))]
        out.append(per[c][at[c]])
        at[c] += 1
        if at[c] == len(per[c]):
            live.remove(c)
            if nxt < conns:
                live.append(nxt)
                nxt += 1
        if rng.random() < 0.02:
            out.append(flowcases.connection_cases()[2])  # a useless packet
    return out
