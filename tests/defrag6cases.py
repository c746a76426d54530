"""IPv6 fragments for the reassembly tests (tests/defrag6_model.py,
gpk_defrag6.h) and tools/defrag6_bench.py: single fragments with chosen header
fields behind optional extension headers, UDP datagrams with a correct
checksum cut into fragments, and random fragmented traffic with reordering,
duplicates and drops."""
import struct

import numpy as np

import flowcases

A = bytes.fromhex("20010db8000000000000000000000001")
B = bytes.fromhex("20010db8000000000000000000000002")
C = bytes.fromhex("20010db80000000000000000000000c3")


def ext(nh, kind):
    """An 8-byte extension header whose Next Header is nh: HopByHop and
    Destination hold one PadN option, Routing is type 0 with no segments."""
    return bytes([nh, 0, 1, 4, 0, 0, 0, 0]) if kind in (0, 60) else bytes([nh, 0, 0, 0, 0, 0, 0, 0])


def frag6(ident, fo, mf, payload, nh=17, src=A, dst=B, vlan=None, front=(), behind=False, trailer=b"", cut=None,
          version=6, tc=0, flow=0, hlim=64, length=None, res=0, frag_bytes=8):
    """Ethernet (+ one VLAN tag) + IPv6 + the extension headers `front` (any of
    0 HopByHop, 60 Destination, 43 Routing, in that order on the wire) + the
    Fragment header + (behind: a Destination header, part of the fragment's
    payload) + payload + trailer. nh: the Fragment header's Next Header;
    length: the Payload Length field (default: what the bytes are); res: the two
    reserved bits beside M; frag_bytes: how many of the Fragment header's 8 bytes
    are there (fewer: a short header, the payload is left out); cut: the capture
    ends after `cut` bytes."""
    body = bytes(payload)
    if behind:
        body = ext(nh, 60) + body
        nh = 60
    fh = struct.pack(">BBHI", nh, 0, (fo << 3) | (res << 1) | mf, ident)[:frag_bytes]
    chain, nxt = b"", 44
    for kind in reversed(front):
        chain = ext(nxt, kind) + chain
        nxt = kind
    rest = chain + fh + (body if frag_bytes == 8 else b"")
    if length is None:
        length = len(rest)
    ip = struct.pack(">IHBB16s16s", (version & 15) << 28 | tc << 20 | flow, length & 0xFFFF, nxt, hlim, src, dst)
    eth = b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02"
    eth += (b"\x81\x00" + struct.pack(">H", vlan) + b"\x86\xdd") if vlan is not None else b"\x86\xdd"
    f = eth + ip + rest + bytes(trailer)
    return f if cut is None else f[:cut]


def udp_segment(src, dst, sport, dport, body):
    """UDP header + body with the checksum over the IPv6 pseudo-header."""
    ln = 8 + len(body)
    seg = bytearray(struct.pack(">HHHH", sport, dport, ln, 0) + bytes(body))
    ck = flowcases.csum(bytes(src) + bytes(dst) + struct.pack(">IHBB", ln, 0, 0, 17) + bytes(seg) +
                        (b"\x00" if ln & 1 else b""))
    struct.pack_into(">H", seg, 6, ck or 0xFFFF)
    return bytes(seg)


def fragments(ident, l4, per=1448, src=A, dst=B, nh=17, **kw):
    """The IPv6 fragments of one datagram whose fragmentable part is l4, `per` bytes each (a multiple of 8)."""
    out = []
    for o in range(0, max(len(l4), 1), per):
        out.append(frag6(ident, o // 8, 1 if o + per < len(l4) else 0, l4[o:o + per], nh=nh, src=src, dst=dst, **kw))
    return out


def body(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def in_order(ident, k, rng, per=8, last=5):
    """k fragments of `per` bytes, the final one of `last` bytes."""
    return [frag6(ident, j * per // 8, 1 if j + 1 < k else 0, body(rng, per if j + 1 < k else last)) for j in range(k)]


def random_traffic(seed, datagrams, lo=3000, hi=9000, per=1448, window=40, dup=0.02, drop=0.01, vlan_every=5):
    """Fragments of `datagrams` UDP datagrams between a few hosts, keys
    interleaved: each fragment is displaced by up to `window` positions, some
    are duplicated or dropped; every vlan_every-th datagram is VLAN-tagged (0:
    none). tests/defragcases.random_traffic's shape as IPv6."""
    rng = np.random.default_rng(seed)
    items = []
    pos = 0.0
    for d in range(datagrams):
        src = A[:14] + bytes([int(rng.integers(0, 4)), int(rng.integers(1, 250))])
        dst = B[:15] + bytes([int(rng.integers(1, 250))])
        l4 = udp_segment(src, dst, 1024 + d % 50000, 4000, body(rng, int(rng.integers(lo, hi))))
        for f in fragments(0x10000 + d, l4, per, src, dst, **({"vlan": 7} if vlan_every and d % vlan_every == 0 else {})):
            if rng.random() < drop:
                continue
            items.append((pos + rng.random() * window, f))
            if rng.random() < dup:
                items.append((pos + rng.random() * window, f))
            pos += 1.0
    items.sort(key=lambda t: t[0])
    return [f for _, f in items]


def quirk_cases():
    """name -> (packets, expected verdicts with 0.. for datagrams, expected
    payloads of the datagrams): Q1-Q9 of the reassembly, each worked out by hand
    from ip6defrag/defrag.go:82-178."""
    H = -32
    atom = frag6(1, 0, 0, b"a" * 11)
    p8 = [bytes([0x41 + k]) * 8 for k in range(4)]
    return {
        # Q1 the first call only stores, even a fragment that is whole; the same packet again returns it
        "Q1 lone atomic fragment": ([atom, atom], [H, 0], [b"a" * 11]),
        # Q2 nothing is removed: a duplicate and a fragment behind the final one both return the datagram again
        "Q2 returned again": ([frag6(2, 0, 1, p8[0]), frag6(2, 1, 0, p8[1]), frag6(2, 1, 0, p8[1]),
                               frag6(2, 5, 0, p8[2]), frag6(2, 0, 1, p8[3])],
                              [H, 0, 1, 2, 3], [p8[0] + p8[1]] * 4),
        # Q3 the key ignores addresses: A's header fields, B's bytes and next header
        "Q3 two hosts one id": ([frag6(3, 0, 1, p8[0], src=A, dst=B, nh=17, hlim=9, tc=3, flow=0x12345),
                                 frag6(3, 1, 0, p8[1], src=C, dst=A, nh=6, hlim=200)], [H, 0], [p8[0] + p8[1]]),
        # Q4 NextHeader is the last fragment's
        "Q4 next header of the last": ([frag6(4, 0, 1, p8[0], nh=17), frag6(4, 1, 0, p8[1], nh=6)], [H, 0],
                                       [p8[0] + p8[1]]),
        # Q5 completeness is not monotone: 0+2 == 2 completes, then offset 1 goes between and 0+2 != 1
        "Q5 not monotone": ([frag6(5, 0, 1, p8[0] * 2), frag6(5, 2, 0, p8[1]), frag6(5, 1, 1, p8[2])], [H, 0, H],
                            [p8[0] * 2 + p8[1]]),
        # Q6 floor division: 12 bytes count as one unit
        "Q6 floor division": ([frag6(6, 0, 1, b"x" * 12), frag6(6, 1, 0, p8[1])], [H, 0], [b"x" * 12 + p8[1]]),
        # Q7 a middle fragment with M = 0 ends the datagram there
        "Q7 final in the middle": ([frag6(7, 0, 1, p8[0]), frag6(7, 1, 0, p8[1]), frag6(7, 2, 0, p8[2])], [H, 0, 1],
                                   [p8[0] + p8[1]] * 2),
        # Q8 reversed arrival: nil until offset 0 arrives
        "Q8 reversed": ([frag6(8, 2, 0, p8[2]), frag6(8, 1, 1, p8[1]), frag6(8, 0, 1, p8[0])], [H, H, 0],
                        [p8[0] + p8[1] + p8[2]]),
        # Q9 an empty MF fragment at offset 0 can never be followed (0 + 0 != any later offset)
        "Q9 empty first fragment": ([frag6(9, 0, 1, b""), frag6(9, 1, 0, p8[1]), frag6(9, 0, 1, p8[0])], [H, H, H], []),
    }
