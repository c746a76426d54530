"""Fragments for the reassembly tests (tests/defrag_model.py, gpk_defrag.h) and
tools/defrag_bench.py: single fragments with chosen header fields, UDP
datagrams with a correct checksum cut at an MTU, and random fragmented traffic
with reordering, duplicates, drops and corrupted fields."""
import struct

import numpy as np

import flowcases

A, B = (10, 1, 0, 1), (10, 1, 0, 2)
PING1 = ["testPing1Frag1", "testPing1Frag2", "testPing1Frag3", "testPing1Frag4"]
PING2 = ["testPing2Frag1", "testPing2Frag2", "testPing2Frag3", "testPing2Frag4"]


def frag(ident, fo, mf, payload, src=A, dst=B, ihl=5, vlan=None, length=None, pad=0, proto=17, cut=None, ttl=64):
    """Ethernet (+ one VLAN tag) + IPv4 (options: NOPs up to ihl) + payload.
    length: the Total Length field (default: what the bytes are); pad: Ethernet
    padding after the IP packet; cut: the capture ends after `cut` bytes."""
    hl = ihl * 4
    if length is None:
        length = hl + len(payload)
    ip = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, 0, length & 0xFFFF, ident, mf << 13 | fo, ttl, proto, 0,
                               bytes(src), bytes(dst)) + b"\x01" * (hl - 20))
    struct.pack_into(">H", ip, 10, flowcases.csum(ip))
    eth = b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02"
    eth += (b"\x81\x00" + struct.pack(">H", vlan) + b"\x08\x00") if vlan is not None else b"\x08\x00"
    f = eth + bytes(ip) + bytes(payload) + b"\x00" * pad
    return f if cut is None else f[:cut]


def udp_segment(src, dst, sport, dport, body):
    """UDP header + body with the checksum over the IPv4 pseudo-header."""
    ln = 8 + len(body)
    seg = bytearray(struct.pack(">HHHH", sport, dport, ln, 0) + bytes(body))
    ck = flowcases.csum(bytes(src) + bytes(dst) + struct.pack(">BBH", 0, 17, ln) + bytes(seg))
    struct.pack_into(">H", seg, 6, ck or 0xFFFF)
    return bytes(seg)


def fragments(ident, l4, per=1480, src=A, dst=B, **kw):
    """The IPv4 fragments of one datagram whose payload is l4, `per` bytes each (a multiple of 8)."""
    out = []
    for o in range(0, max(len(l4), 1), per):
        out.append(frag(ident, o // 8, 1 if o + per < len(l4) else 0, l4[o:o + per], src=src, dst=dst, **kw))
    return out


def body(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def random_traffic(seed, datagrams, lo=3000, hi=9000, per=1480, window=40, dup=0.05, drop=0.05, corrupt=0.02):
    """Fragments of `datagrams` UDP datagrams between a few hosts, keys
    interleaved: each fragment is displaced by up to `window` positions, some
    are duplicated, dropped, or get a wrong Length or offset."""
    rng = np.random.default_rng(seed)
    items = []
    pos = 0.0
    for d in range(datagrams):
        src = (10, 2, int(rng.integers(0, 4)), int(rng.integers(1, 250)))
        dst = (10, 3, 0, int(rng.integers(1, 250)))
        l4 = udp_segment(src, dst, 1024 + d % 50000, 4000, body(rng, int(rng.integers(lo, hi))))
        for f in fragments(d & 0xFFFF, l4, per, src, dst):
            r = rng.random()
            if r < drop:
                continue
            if r < drop + corrupt:
                b = bytearray(f)
                if rng.integers(0, 2):  # Length: tiny (securityChecks) or anything
                    struct.pack_into(">H", b, 16, int(rng.integers(20, 40) if rng.integers(0, 2) else
                                                      rng.integers(40, 3000)))
                else:                   # the offset, somewhere in or just past the datagram; MF kept
                    ff = struct.unpack_from(">H", b, 20)[0]
                    struct.pack_into(">H", b, 20, (ff & 0x2000) | int(rng.integers(0, 2 * len(l4) // 8)))
                f = bytes(b)
            items.append((pos + rng.random() * window, f))
            if rng.random() < dup:
                items.append((pos + rng.random() * window, f))
            pos += 1.0
    items.sort(key=lambda t: t[0])
    return [f for _, f in items]


def quirk_cases():
    """name -> (packets, expected verdicts with 0.. for datagrams, expected pending): build's branches,
    worked out by hand from defrag.go:214-326."""
    H, HOLE, INV, PANIC = -16, -17, -18, -20
    x, w, z, y = frag(2, 0, 1, b"x" * 24), frag(2, 1, 1, b"w" * 8), frag(2, 5, 0, b"z" * 8), frag(2, 2, 1, b"y" * 8)
    return {
        # MF offset 0 / 64 bytes, then MF offset 32 / 16 bytes: no larger entry, so not listed, yet Current = 80
        "counted, not listed": ([frag(7, 0, 1, b"a" * 64), frag(7, 4, 1, b"b" * 16)], [H, H], [0, 1]),
        # 0..16 listed, 8..24 counted only, final 32..40: Highest 40 == Current 40, build finds 32 > 16
        "hole": ([frag(1, 0, 1, b"a" * 16), frag(1, 1, 1, b"b" * 16), frag(1, 4, 0, b"c" * 8)], [H, H, HOLE], [0, 1, 2]),
        # x 0..24, w counted only, z 40..48 final, y 16..24 inserted before z: Highest 48 == Current 48; build
        # takes y from startAt 8 and adds y's OFFSET 16 to currentOffset (24 -> 40), which lands on z
        "overlap that completes": ([x, w, z, y], [H, H, H, 0], []),
        # the same with y's capture cut 4 bytes into its payload: Payload[8:] panics
        "panic": ([x, w, z, frag(2, 2, 1, b"y" * 8, cut=14 + 20 + 4)], [H, H, H, PANIC], [0, 1, 2, 3]),
        # final 24..32 first, then 0..32: Current 40 never equals Highest 32
        "overlap that never completes": ([frag(3, 3, 0, b"f" * 8), frag(3, 0, 1, b"g" * 32)], [H, H], [0, 1]),
        # x 0..24, 24..40, then an empty final fragment at 16 inserted between: startAt 8 > Length-20 = 0
        "invalid fragment": ([x, frag(2, 3, 1, b"v" * 16), frag(2, 2, 0, b"")], [H, H, INV], [0, 1, 2]),
        # a duplicate offset is ignored before (never pending) and after completion (a new list)
        "duplicates": ([frag(4, 0, 1, b"p" * 16), frag(4, 0, 1, b"q" * 16), frag(4, 2, 0, b"r" * 5),
                        frag(4, 2, 0, b"r" * 5)], [H, H, 0, H], [3]),
    }
