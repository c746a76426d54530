"""Hand-derived ICMPv4 / ICMPv6 / ICMPv6Echo / ARP packets, one per quirk of
include/gpk_control.h, and the seeded corpus of the control
tests.

Every case is (name, packet bytes). The expected values come from
control_model.py; the cases that pin a quirk also carry the expected outcome by
hand in EXPECT (appended layer types, error code and arguments, the type
returned as unsupported, status bits), derived from the reference's source, so
the model is checked too.

The parser routes three private EtherTypes straight to ICMPv6, ICMPv4 and
ICMPv6Echo (gpk_parser_set_ethertype): the only way to a control layer without a
network layer, to an ICMPv4 message longer than an IPv4 datagram, and to an
ICMPv6Echo in front.
"""
import random
import struct

from tunnelcases import MAC, dot1q, eth, ip4, ip6, tcp, udp, vxlan, over_udp, VX  # noqa: F401

ET_ICMP6, ET_ICMP4, ET_ECHO = 0x9998, 0x9997, 0x9996
EDITS = {ET_ICMP6: 57, ET_ICMP4: 19, ET_ECHO: 132}
PARSER = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"],
              ethertype=EDITS)
PARSER_IGNORE = dict(PARSER, ignore_unsupported=True)
PARSER_NOPAYLOAD = dict(PARSER, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP"])
SRC4, DST4 = b"\x0a\x00\x00\x01", b"\x0a\x00\x00\x02"   # tunnelcases.ip4's addresses
SRC6, DST6 = bytes(15) + b"\x01", bytes(15) + b"\x02"   # tunnelcases.ip6's addresses


def csum16(data, start=0):
    s = start
    for i in range(0, len(data) - 1, 2):
        s += data[i] << 8 | data[i + 1]
    if len(data) & 1:
        s += data[-1] << 8
    while s > 0xffff:
        s = (s >> 16) + (s & 0xffff)
    return ~s & 0xffff


def icmp4(body=b"ping-payload", typ=8, code=0, ident=0x1234, seq=7, good=True):
    m = struct.pack(">BBHHH", typ, code, 0, ident, seq) + body
    c = csum16(m)
    if not good:
        c ^= 0x0100
    return m[:2] + struct.pack(">H", c) + m[4:]


def icmp6(body=b"", typ=128, code=0, addresses=SRC6 + DST6, good=True):
    """An ICMPv6 message whose checksum holds for the pseudo-header of `addresses`."""
    m = struct.pack(">BBH", typ, code, 0) + body
    ph = 0
    for i in range(0, len(addresses), 2):
        ph += addresses[i] << 8 | addresses[i + 1]
    c = csum16(m, ph + 58 + (len(m) & 0xffff) + (len(m) >> 16))
    if not good:
        c ^= 0x0001
    return m[:2] + struct.pack(">H", c) + m[4:]


def echo6(ident=0xbeef, seq=3, data=b"abcdefgh", typ=128, **kw):
    return icmp6(struct.pack(">HH", ident, seq) + data, typ, **kw)


def arp(op=1, hw=6, prot=4, htype=1, ptype=0x0800, fill=None):
    adr = bytes((0x10 + i) & 0xff for i in range(2 * hw + 2 * prot)) if fill is None else fill
    return struct.pack(">HHBBH", htype, ptype, hw, prot, op) + adr


def hbh(nh, opts=b"\x01\x04\x00\x00\x00\x00"):
    assert (2 + len(opts)) % 8 == 0
    return bytes([nh, (2 + len(opts)) // 8 - 1]) + opts


def ext(nh, words=0):
    """A Routing / Destination header of 8 + 8 * words bytes."""
    return bytes([nh, words]) + bytes(6 + 8 * words)


def quirk_cases():
    c = []
    E = {}

    def add(name, pkt, **expect):
        c.append((name, pkt))
        if expect:
            E[name] = expect
    # ---- ICMPv4 (icmp4.go:221-232)
    add("icmp4_echo", eth(ip4(icmp4(), 1)), cls=0, lts=[19, 2], status=2 | 4, contents=8, payload=12, id=0x1234, seq=7,
        typecode=0x0800)
    add("icmp4_bad_checksum", eth(ip4(icmp4(good=False), 1)), cls=0, lts=[19, 2], status=2)
    add("icmp4_odd_length", eth(ip4(icmp4(b"odd"), 1)), cls=0, status=2 | 4, payload=3)
    add("icmp4_len7", eth(ip4(icmp4()[:7], 1)), cls=3, err=80, status=1, lts=[])
    add("icmp4_len8_empty_payload", eth(ip4(icmp4(b""), 1)), cls=0, lts=[19], status=2 | 4, payload=0, unsupported=0)
    add("icmp4_unreachable", eth(ip4(icmp4(ip4(udp(b"", 1, 2), 17), typ=3, code=3, ident=0, seq=0), 1)), lts=[19, 2],
        typecode=0x0303)
    # P9: IPv4 Length 0 (TSO): the length is the slice's, so the whole message is there
    add("icmp4_tso_length0", eth(ip4(icmp4(bytes(range(200))), 1, total=0)), cls=0, lts=[19, 2], status=2 | 4, payload=200)
    add("icmp4_in_fragment", eth(ip4(icmp4(), 1)[:6] + b"\x20\x00" + ip4(icmp4(), 1)[8:]))  # MF: not a candidate
    add("icmp4_padded_frame", eth(ip4(icmp4(b""), 1)) + bytes(18), lts=[19], payload=0)  # IPv4 trims the padding
    add("icmp4_dot1q", MAC + struct.pack(">H", 0x8100) + dot1q(ip4(icmp4(), 1)), cls=0, lts=[19, 2])
    add("icmp4_no_network_layer", eth(icmp4(b"direct"), ET_ICMP4), cls=0, lts=[19, 2], status=2 | 4)
    # ---- ICMPv6 (icmp6.go:189-198, :230-261)
    add("icmp6_echo_request", eth(ip6(echo6(), 58), 0x86dd), cls=1, lts=[57, 132], status=2 | 4, contents=4, payload=12,
        id=0xbeef, seq=3, unsupported=0, next=132)
    add("icmp6_echo_reply_bad_checksum", eth(ip6(echo6(typ=129, good=False), 58), 0x86dd), lts=[57, 132], status=2)
    # the Echo sets no BaseLayer: the loop ends after it whatever follows
    add("icmp6_echo_long_data", eth(ip6(echo6(data=bytes(300)), 58), 0x86dd), lts=[57, 132], payload=304, err=0)
    add("icmp6_echo_3_bytes", eth(ip6(icmp6(b"\x00\x01\x02"), 58), 0x86dd), cls=1, lts=[57], err=82, status=1 | 2 | 4)
    add("icmp6_echo_4_bytes", eth(ip6(icmp6(b"\x00\x01\x00\x02"), 58), 0x86dd), lts=[57, 132], id=1, seq=2)
    add("icmp6_len3", eth(ip6(icmp6()[:3], 58), 0x86dd), cls=3, err=81, status=1, lts=[])
    add("icmp6_len4_echo_type", eth(ip6(icmp6(), 58), 0x86dd), cls=1, lts=[57], payload=0, unsupported=0, status=2 | 4)
    add("icmp6_dest_unreachable", eth(ip6(icmp6(bytes(4) + b"orig", 1), 58), 0x86dd), lts=[57, 2], next=2)
    for typ, nxt, nm in ((133, 124, "router_solicitation"), (134, 125, "router_advertisement"),
                         (135, 126, "neighbor_solicitation"), (136, 127, "neighbor_advertisement"),
                         (137, 128, "redirect"), (131, 135, "mld1_report"), (132, 136, "mld1_done"),
                         (143, 138, "mld2_report")):
        add("icmp6_" + nm, eth(ip6(icmp6(bytes(20), typ), 58), 0x86dd), cls=1, lts=[57], unsupported=nxt, next=nxt,
            status=2 | 4)
    add("icmp6_mld_query_payload_20", eth(ip6(icmp6(bytes(20), 130), 58), 0x86dd), lts=[57], unsupported=137)
    add("icmp6_mld_query_payload_21", eth(ip6(icmp6(bytes(21), 130), 58), 0x86dd), lts=[57], unsupported=139)
    add("icmp6_behind_hopbyhop", eth(ip6(hbh(58) + echo6(), 0), 0x86dd), cls=1, lts=[57, 132], status=2 | 4)
    add("icmp6_behind_skipper_chain", eth(ip6(ext(60) + ext(58, 1) + echo6(), 43), 0x86dd), cls=1, lts=[57, 132],
        status=2 | 4, hdr=14 + 40 + 8 + 16)
    # the pseudo-header is the last network layer's, here an IPv4's four-byte addresses
    add("icmp6_inside_ipv4", eth(ip4(echo6(addresses=SRC4 + DST4), 58)), cls=1, lts=[57, 132], status=2 | 4)
    add("icmp6_inside_ipv4_with_ipv6_sum", eth(ip4(echo6(), 58)), cls=1, status=2)
    add("icmp6_ip6_in_ip4", eth(ip4(ip6(echo6(), 58), 41)), cls=1, lts=[57, 132], status=2 | 4)
    # no network layer (a table edit): no sum, computeChecksum's error
    add("icmp6_no_network_layer", eth(echo6(), ET_ICMP6), cls=1, lts=[57, 132], status=8)
    add("echo_in_front", eth(struct.pack(">HH", 9, 10) + b"rest", ET_ECHO), cls=1, lts=[132], id=9, seq=10, contents=0,
        payload=0, status=0)
    add("echo_in_front_3_bytes", eth(b"\x00\x09\x00", ET_ECHO), cls=3, err=82, status=1)
    # ---- ARP (arp.go:42-67)
    add("arp_request_42", eth(arp(), 0x0806), cls=2, lts=[10], contents=28, payload=0, op=1, hw=6, prot=4)
    # Ethernet trims 802.3 frames only: the padding of a 60-byte frame is ARP's payload
    add("arp_reply_padded_60", eth(arp(2), 0x0806) + bytes(18), cls=2, lts=[10, 2], contents=28, payload=18, op=2)
    add("arp_len7", eth(arp()[:7], 0x0806), cls=3, err=83, a0=7, status=1)
    add("arp_sizes_exceed_slice", eth(arp(hw=255, prot=4, fill=bytes(20)), 0x0806), cls=3, err=84, a0=28, a1=526, status=1)
    add("arp_one_byte_short", eth(arp()[:27], 0x0806), cls=3, err=84, a0=27, a1=28)
    add("arp_zero_sizes", eth(arp(hw=0, prot=0) + b"tail", 0x0806), cls=2, lts=[10, 2], contents=8, payload=4)
    add("arp_dot1q", MAC + struct.pack(">H", 0x8100) + dot1q(arp(), 0x0806), cls=2, lts=[10])
    # ---- not candidates
    add("plain_tcp", eth(ip4(tcp(b"hello"), 6)))
    add("plain_udp", eth(ip4(udp(bytes(12), 50004, 53), 17)))
    add("icmp4_empty_ip_payload", eth(ip4(b"", 1)))  # an empty payload ends the loop before the type is looked at
    return c, E


def layers17():
    """Ethernet, 14 Dot1Q tags, IPv4: 16 layers, ICMPv4 would be the 17th; and one tag more."""
    tags = lambda n: MAC + b"".join(b"\x81\x00" + b"\x00\x05" for _ in range(n)) + b"\x08\x00"  # noqa: E731
    return tags(14) + ip4(icmp4(), 1), tags(15) + ip4(icmp4(), 1)


def fuzz_packets(seed, n):
    """Valid encapsulations with mutated control-header bytes and random
    truncation, aimed at the headers' own length boundaries."""
    rnd = random.Random(seed)
    out = []
    types6 = [128, 129, 1, 2, 3, 130, 131, 132, 133, 134, 135, 136, 137, 143, 200]
    for _ in range(n):
        k = rnd.randrange(12)
        good = rnd.random() < 0.7
        if k < 4:
            msg = icmp4(bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 0, 1, 7, 8, 33, 100]))),
                        typ=rnd.choice([0, 3, 8, 11]), good=good)
            hdr = 8
            wrap = rnd.choice([lambda m: eth(ip4(m, 1)),
                               lambda m: eth(ip4(m, 1)) + bytes(rnd.randrange(0, 20)),
                               lambda m: eth(m, ET_ICMP4)])
        elif k < 9:
            typ = rnd.choice(types6)
            body = bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 1, 3, 4, 8, 19, 20, 21, 24, 60])))
            v4 = rnd.random() < 0.15
            msg = icmp6(body, typ, addresses=SRC4 + DST4 if v4 else SRC6 + DST6, good=good)
            hdr = 8
            r = rnd.random()
            if v4:
                wrap = lambda m: eth(ip4(m, 58))  # noqa: E731
            elif r < 0.15:
                wrap = lambda m: eth(m, ET_ICMP6)  # noqa: E731
            elif r < 0.3:
                wrap = lambda m: eth(ip6(hbh(58) + m, 0), 0x86dd)  # noqa: E731
            elif r < 0.4:
                wrap = lambda m: eth(ip6(ext(58, rnd.randrange(3)) + m, rnd.choice([43, 60])), 0x86dd)  # noqa: E731
            else:
                wrap = lambda m: eth(ip6(m, 58), 0x86dd)  # noqa: E731
        elif k < 11:
            hw, prot = rnd.choice([(6, 4), (6, 4), (6, 16), (0, 0), (8, 4), (255, 255), (20, 1)])
            msg = arp(rnd.choice([1, 2]), hw, prot) + bytes(rnd.choice([0, 0, 18, 3]))
            hdr = 8
            wrap = lambda m: eth(m, 0x0806)  # noqa: E731
        else:
            msg = struct.pack(">HH", rnd.randrange(65536), rnd.randrange(65536)) + bytes(rnd.randrange(6))
            hdr = 4
            wrap = lambda m: eth(m, ET_ECHO)  # noqa: E731
        msg = bytearray(msg)
        if rnd.random() < 0.4 and msg:
            for _ in range(rnd.randrange(1, 3)):
                msg[rnd.randrange(min(len(msg), hdr))] = rnd.randrange(256)
        msg = bytes(msg)
        r = rnd.random()
        if r < 0.3:     # cut near the header's end
            pkt = wrap(msg[:rnd.randrange(0, min(len(msg), hdr + 6) + 1)])
        elif r < 0.4:   # cut anywhere in the whole packet
            pkt = wrap(msg)
            pkt = pkt[:rnd.randrange(1, len(pkt) + 1)]
        else:
            pkt = wrap(msg)
        out.append(pkt)
    return out


FUZZ_SEED = 20261021
FUZZ_N = 4096
