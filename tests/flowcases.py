"""Packets for the flow-keyed grouping tests (row (f)3): ip4defrag's own test
frames, frames built from the field values of its struct-based tests, and
TCP segments covering tcpassembly's "useless packet" filter."""
import json
import os
import struct

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# statsassembly + Fragment: the parser a defragmenting consumer would run
DEFRAG_PARSER = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"])


def defrag_frames():
    g = json.load(open(os.path.join(GOLD, "defrag_frames.json")))
    return {k: bytes.fromhex(v) for k, v in g["frames"].items()}, g["same_datagram"]


def csum(b):
    s = 0
    for k in range(0, len(b) - 1, 2):
        s += b[k] << 8 | b[k + 1]
    if len(b) & 1:
        s += b[-1] << 8
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def eth_ip4(src, dst, ident, flags, frag_off, length, proto=1, payload=b"", ttl=15, total=None):
    """Ethernet + IPv4 header with the given field values (Length may disagree with the bytes)."""
    ip = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, 0, length, ident, flags << 13 | frag_off, ttl, proto, 0,
                               bytes(src), bytes(dst)))
    struct.pack_into(">H", ip, 10, csum(ip))
    frame = b"\x00\x11\x22\x33\x44\x55\x66\x77\x88\x99\xaa\xbb\x08\x00" + bytes(ip) + payload
    if total is not None:
        frame = frame[:total] + b"\x00" * max(0, total - len(frame))
    return frame


def defrag_struct_cases():
    """(label, frame): the field values of defrag_test.go's struct-based tests."""
    a, b = (1, 1, 1, 1), (2, 2, 2, 2)
    MF, DF = 1, 2
    return [
        ("TestNotFrag (DF)", eth_ip4(a, b, 0, DF, 0, 20)),
        ("TestDefragTooSmall Length 27 MF", eth_ip4(a, b, 0xcc, MF, 0, 27, payload=b"x" * 7)),
        ("TestDefragTooSmall Length 28 MF", eth_ip4(a, b, 0xcc, MF, 0, 28, payload=b"x" * 8)),
        ("TestDefragSmallFinalFragment", eth_ip4(a, b, 0xcc, 0, 0, 27, payload=b"x" * 7)),
        ("TestDefragFragmentOffset 0", eth_ip4(a, b, 0xcc, MF, 0, 512, payload=b"y" * 492)),
        ("TestDefragFragmentOffset 8184", eth_ip4(a, b, 0xcc, MF, 8184, 512, payload=b"y" * 492)),
        ("TestDefragMaxSize Length 65535", eth_ip4(a, b, 0xcc, MF, 0, 65535, payload=b"z" * 100)),
        ("TestDefragMaxSize Length 28 off 1", eth_ip4(a, b, 0xcc, MF, 1, 28, payload=b"z" * 8)),
        ("last fragment, offset 8183", eth_ip4(a, b, 0xcd, 0, 8183, 28, payload=b"z" * 8)),
        ("TSO Length 0 with MF", eth_ip4(a, b, 0xce, MF, 0, 0, payload=b"w" * 40)),
        ("Length 0, IHL 5, short", eth_ip4(a, b, 0xcf, MF, 3, 0, payload=b"w" * 2)),
    ]


def tcp_segment(src, dst, sport, dport, flags, payload=b"", v6=False, pad=0):
    tcp = struct.pack(">HHIIBBHHH", sport, dport, 1, 0, 5 << 4, flags, 512, 0, 0) + payload
    if v6:
        ip = struct.pack(">IHBB16s16s", 0x60000000, len(tcp), 6, 64, bytes(src), bytes(dst))
        et = b"\x86\xdd"
    else:
        ip = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, 0, 20 + len(tcp), 1, 0x4000, 64, 6, 0, bytes(src), bytes(dst)))
        struct.pack_into(">H", ip, 10, csum(ip))
        et = b"\x08\x00"
    return b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02" + et + bytes(ip) + tcp + b"\x00" * pad


def connection_cases():
    a4, b4 = (10, 0, 0, 1), (10, 0, 0, 2)
    a6, b6 = bytes(range(16)), bytes(range(16, 32))
    SYN, FIN, RST, ACK, PSH = 2, 1, 4, 16, 8
    return [
        tcp_segment(a4, b4, 1000, 2000, SYN),
        tcp_segment(b4, a4, 2000, 1000, SYN | ACK),          # the other direction: its own key
        tcp_segment(a4, b4, 1000, 2000, ACK),                 # useless: no flags, no payload
        tcp_segment(a4, b4, 1000, 2000, ACK, pad=10),         # Ethernet padding is not payload
        tcp_segment(a4, b4, 1000, 2000, ACK | PSH, b"hello"),
        tcp_segment(a6, b6, 1000, 2000, ACK | PSH, b"v6 data", v6=True),
        tcp_segment(a6, b6, 1000, 2000, FIN | ACK, v6=True),
        tcp_segment(a4, b4, 1000, 2001, RST),
        tcp_segment(a4, b4, 1000, 2000, FIN | ACK),
    ]


# ---------------------------------------------------------------------------
# key derivation at the edges (tests/test_flows_keys_gpu.py): header stacks
# that put the key's bytes (addresses, ports, TCP flags, IPv4 Id) across and
# beyond the fused kernel's header window, the 16-inline-codes boundary,
# IP-in-IP, and the "useless packet" filter at data offset 15.

MAC = b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02"
SYN, FIN, RST, PSH, ACK = 2, 1, 4, 8, 16


def ether(tags, ethertype):
    """Ethernet header with `tags` stacked 802.1Q tags in front of `ethertype`."""
    out = MAC
    for k in range(tags):
        out += b"\x81\x00" + struct.pack(">H", 100 + k)
    return out + struct.pack(">H", ethertype)


def ip4(src, dst, proto, payload, ihl=5, ident=1, ff=0x4000):
    """IPv4 header of `ihl` dwords (No-Operation options) in front of payload."""
    h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, 0, 4 * ihl + len(payload), ident, ff, 64, proto, 0,
                              bytes(src), bytes(dst)) + b"\x01" * (4 * (ihl - 5)))
    struct.pack_into(">H", h, 10, csum(h))
    return bytes(h) + payload


def ip6(src, dst, nh, payload, dstopts=0):
    """IPv6 header, then a Destination Options header of `dstopts` bytes (Pad1 options) if any."""
    ext = bytes([nh, dstopts // 8 - 1]) + b"\x00" * (dstopts - 2) if dstopts else b""
    return struct.pack(">IHBB16s16s", 0x60000000, len(ext) + len(payload), 60 if dstopts else nh, 64, bytes(src),
                       bytes(dst)) + ext + payload


def tcp(sport, dport, flags, payload=b"", doff=5, opts=None):
    if opts is None:
        opts = b"\x01" * (4 * (doff - 5))
    return struct.pack(">HHIIBBHHH", sport, dport, 1, 0, doff << 4, flags, 512, 0, 0) + opts + payload


def v6addr(a, b):
    return bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(10) + bytes([a, b])


def _flows6(lid):
    """Six (src, dst, sport, dport) of one layout: three flows of two packets;
    the second flow differs from the first only in the last port byte, the
    third only in the last destination-address byte."""
    a, b = lid >> 8, lid & 255
    base = ((10, 9, a, b), (10, 8, 0, 1), 1000, 0x5000)
    port = (base[0], base[1], 1000, 0x5001)
    addr = (base[0], (10, 8, 0, 0), 1000, 0x5000)
    return [base, port, addr, base, port, addr]


def window_connection4():
    """TCP/IPv4 behind 0-13 802.1Q tags with IHL 5-15: the TCP header starts at
    every offset 34, 38, .. 126. -> [(tcp start, packet)]"""
    out = []
    for tags in range(14):
        for ihl in range(5, 16):
            for j, (s, d, sp, dp) in enumerate(_flows6(tags * 16 + ihl)):
                seg = tcp(sp, dp, SYN if j < 3 else ACK | PSH, b"data%d" % j)
                out.append((14 + 4 * tags + 4 * ihl, ether(tags, 0x0800) + ip4(s, d, 6, seg, ihl=ihl)))
    return out


def window_connection4in4():
    """TCP behind IPv4 in IPv4 (outer IHL 5-15, 0-4 tags): the inner header
    starts at 34 .. 90, so its addresses (inner + 12 .. + 19) lie before, across
    and beyond byte 96 (which the Ethernet + tags + IPv4 sweep cannot reach
    within 16 layers). -> [(inner IPv4 start, packet)]"""
    out = []
    for tags in range(5):
        for ihl in range(5, 16):
            for j, (s, d, sp, dp) in enumerate(_flows6(0x1000 + tags * 16 + ihl)):
                inner = ip4(s, d, 6, tcp(sp, dp, SYN if j < 3 else ACK | PSH, b"x" * j))
                pkt = ether(tags, 0x0800) + ip4((172, 16, 0, j), (172, 16, 1, 1), 4, inner, ihl=ihl)
                out.append((14 + 4 * tags + 4 * ihl, pkt))
    return out


def window_connection6():
    """TCP/IPv6 behind a Destination Options header of 0, 8, 48, 56, 64, 248 or
    2048 bytes, under 0, 10, 11 or 12 tags (the destination address's last
    dword crosses byte 96 at 11). -> [(tcp start, packet)]"""
    out = []
    for tags in (0, 10, 11, 12):
        for k, ext in enumerate((0, 8, 48, 56, 64, 248, 2048)):
            for j, (s, d, sp, dp) in enumerate(_flows6(tags * 8 + k)):
                seg = tcp(sp, dp, SYN if j < 3 else ACK | PSH, b"six%d" % j)
                pkt = ether(tags, 0x86dd) + ip6(v6addr(s[2], s[3]), v6addr(0, d[3]), 6, seg, dstopts=ext)
                out.append((14 + 4 * tags + 40 + ext, pkt))
    return out


def window_defrag():
    """MF fragments behind 0-24 tags with IHL 5-15: the IPv4 header starts at
    14 .. 110, so Id (ip + 4), source (ip + 12) and destination (ip + 16) lie
    before, across and beyond byte 96. Three datagrams of two fragments per
    layout: the second differs from the first only in Id's low byte, the third
    only in the last destination-address byte. -> [(ip start, packet)]"""
    out = []
    for tags in range(25):
        for ihl in range(5, 16):
            lid = tags * 16 + ihl
            src = (10, 7, lid >> 8, lid & 255)
            keys = [((10, 6, 0, 1), 0x1200), ((10, 6, 0, 1), 0x1201), ((10, 6, 0, 0), 0x1200)]
            for j, (dst, ident) in enumerate(keys + keys):
                pkt = ether(tags, 0x0800) + ip4(src, dst, 17, b"f" * 16, ihl=ihl, ident=ident,
                                                ff=0x2000 | (0 if j < 3 else 2))
                out.append((14 + 4 * tags, pkt))
    return out


def inline_boundary_cases():
    """(label, packet): TCP as decoded-list entry 14, 15 (the last inline code),
    16 and 17 (past the inline list), and behind IPv4 in IPv4 at 16."""
    a, b = (10, 5, 0, 1), (10, 5, 0, 2)
    out = []
    for tags in (12, 13, 14, 15):
        for sp in (1, 2, 1):
            out.append(("%d tags: IPv4 at %d, TCP at %d" % (tags, tags + 1, tags + 2),
                        ether(tags, 0x0800) + ip4(a, b, 6, tcp(sp, 80, SYN))))
    for tags in (12, 13):
        for sp in (1, 2, 1):
            inner = ip4(a, b, 6, tcp(sp, 80, SYN))
            out.append(("%d tags, 4in4: TCP at %d" % (tags, tags + 3),
                        ether(tags, 0x0800) + ip4(b, a, 4, inner)))
    return out


def ip_in_ip_cases():
    """(label, packet): IPv4 in IPv4, IPv6 in IPv4 and IPv4 in IPv6 before TCP.
    Per combination: the base packet; equal inner and other outer addresses
    (the base's connection); equal outer and other inner addresses (another
    connection). Then IPv4-in-IPv4 fragments for DEFRAG: the outer header a
    fragment and the inner not, and the reverse."""
    o4, o4b, i4, i4b = [(192, 168, 0, k) for k in (1, 2, 3, 4)]
    o6, o6b, i6, i6b = [v6addr(7, k) for k in (1, 2, 3, 4)]
    dst4, dst6 = (192, 168, 9, 9), v6addr(9, 9)
    seg = tcp(5000, 6000, SYN)

    def p44(o, i):
        return ether(0, 0x0800) + ip4(o, dst4, 4, ip4(i, dst4, 6, seg))

    def p64(o, i):
        return ether(0, 0x0800) + ip4(o, dst4, 41, ip6(i, dst6, 6, seg))

    def p46(o, i):
        return ether(0, 0x86dd) + ip6(o, dst6, 4, ip4(i, dst4, 6, seg))

    out = []
    for name, f, o, ob, i, ib in (("4in4", p44, o4, o4b, i4, i4b), ("6in4", p64, o4, o4b, i6, i6b),
                                  ("4in6", p46, o6, o6b, i4, i4b)):
        out += [(name + " base", f(o, i)), (name + " other outer", f(ob, i)), (name + " other inner", f(o, ib)),
                (name + " base again", f(o, i))]
    # the same inner addresses as plain TCP/IPv4: the 4in4 base's connection
    out.append(("plain inner", ether(0, 0x0800) + ip4(i4, dst4, 6, seg)))
    inner_df = ip4(i4, dst4, 17, b"u" * 16, ident=7)
    inner_mf = ip4(i4, dst4, 17, b"u" * 16, ident=7, ff=0x2000)
    for k in range(2):
        out.append(("4in4 outer MF, inner DF", ether(0, 0x0800) + ip4(o4, dst4, 4, inner_df, ident=9, ff=0x2000)))
        out.append(("4in4 outer DF, inner MF", ether(0, 0x0800) + ip4(o4, dst4, 4, inner_mf, ident=9)))
        out.append(("4in4 outer MF, inner MF", ether(0, 0x0800) + ip4(o4, dst4, 4, inner_mf, ident=9, ff=0x2000)))
        out.append(("plain inner MF", ether(0, 0x0800) + inner_mf))
    return out


def useless_filter_cases():
    """(label, packet): the "ignoring useless packet" filter at data offset 15."""
    a, b = (10, 4, 0, 1), (10, 4, 0, 2)

    def pkt(seg, pad=0):
        return ether(0, 0x0800) + ip4(a, b, 6, seg) + b"\x00" * pad

    short = tcp(7, 8, ACK, doff=15, opts=b"")  # 20 bytes that claim a 60-byte header
    return [
        ("ACK, offset 15, options fill the segment", pkt(tcp(7, 8, ACK, doff=15))),
        ("the same with Ethernet padding", pkt(tcp(7, 8, ACK, doff=15), pad=9)),
        ("ACK, offset 15, one payload byte", pkt(tcp(7, 8, ACK, b"!", doff=15))),
        ("ACK | SYN, offset 15, no payload", pkt(tcp(7, 8, ACK | SYN, doff=15))),
        ("ACK, offset 15 in a 20-byte segment", pkt(short)),
        ("ACK | SYN, offset 15 in a 20-byte segment", pkt(tcp(7, 8, ACK | SYN, doff=15, opts=b""))),
        ("ACK, offset 4", pkt(tcp(7, 8, ACK, b"pay", doff=4, opts=b""))),
    ]
