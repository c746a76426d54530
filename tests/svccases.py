"""Hand-derived DHCPv4, DHCPv6 and NTP packets, one per error site, quirk and
layer of include/gpk_svc.h, and the seeded corpus of the
service tests.

Every case is (name, packet bytes). The expected values come from
svc_model.py; EXPECT also carries the outcome by hand (class, layer type, error
code and arguments, status bits, entries, a few fields), derived from the
reference's source, so the model is checked too.

The parser keeps ndpcases' edits (so one parser can hold the control, NDP and
service layers), registers three private UDP ports and one TCP port for the
three layers (RegisterUDPPortLayerType / RegisterTCPPortLayerType) and routes
three private EtherTypes straight to them: the only way to a message longer
than a UDP datagram, which the one run-time panic of the path needs.
"""
import random
import struct

import ndpcases as NC
from tunnelcases import MAC, eth, ip4, ip6, tcp, udp, vxlan, over_udp, VX  # noqa: F401

LT_NTP, LT_DHCP4, LT_DHCP6 = 117, 118, 134
LAYER_TYPES = (LT_DHCP4, LT_DHCP6, LT_NTP)
ET_OF = {lt: 0x9a00 + lt for lt in LAYER_TYPES}          # EtherType -> the layer itself
UDP_EDIT = {9067: LT_DHCP4, 9546: LT_DHCP6, 9123: LT_NTP}  # RegisterUDPPortLayerType
TCP_EDIT = {8067: LT_DHCP4}
PARSER = dict(NC.PARSER, ethertype=dict(list(NC.EDITS.items()) + [(et, lt) for lt, et in ET_OF.items()]),
              udp_port=UDP_EDIT, tcp_port=TCP_EDIT)
PARSER_IGNORE = dict(PARSER, ignore_unsupported=True)
PARSER_NOPAYLOAD = dict(PARSER, decoders=[d for d in PARSER["decoders"] if d != "PAYLOAD"])
PLAIN_PARSER = dict(NC.PARSER)                            # no port edits: the registry's 67, 68, 123, 546, 547 only

HDR = 14 + 20 + 8      # the message's packet offset behind Ethernet, IPv4 and UDP
HDR6 = 14 + 40 + 8
CHADDR = bytes.fromhex("000c29a1b2c3")
MAGIC = bytes.fromhex("63825363")
PAD, END = b"\x00", b"\xff"
DUID = bytes.fromhex("00010001" "1c39cf88" "080027fe8f95")
LINK = bytes.fromhex("20010db8000000000000000000000001")
PEER = bytes.fromhex("fe800000000000000a0027fffefe8f95")


def opt4(typ, data=b"", length=None):
    return bytes([typ, len(data) if length is None else length]) + data


def dhcp4(options=b"", op=1, htype=1, hlen=6, hops=0, xid=0x3903f326, secs=0, flags=0x8000, ciaddr=bytes(4),
          yiaddr=bytes(4), siaddr=bytes(4), giaddr=bytes(4), chaddr=CHADDR, sname=b"", file=b"", magic=MAGIC):
    return (struct.pack(">BBBBIHH", op, htype, hlen, hops, xid, secs, flags) + ciaddr + yiaddr + siaddr + giaddr +
            chaddr.ljust(16, b"\x00") + sname.ljust(64, b"\x00") + file.ljust(128, b"\x00") + magic + options)


def discover(host=b"host-1"):
    """A Discover with eight options, End not counted."""
    return dhcp4(opt4(53, b"\x01") + opt4(61, b"\x01" + CHADDR) + opt4(12, host) + opt4(60, b"MSFT 5.0") +
                 opt4(50, bytes([10, 0, 0, 99])) + opt4(55, bytes([1, 3, 6, 15, 31, 33, 43, 44, 46, 47, 121, 249, 252])) +
                 opt4(57, b"\x05\xdc") + opt4(51, struct.pack(">I", 3600)) + END)


def ack(yiaddr=bytes([10, 0, 0, 99]), server=bytes([10, 0, 0, 1]), lease=86400):
    return dhcp4(opt4(53, b"\x05") + opt4(54, server) + opt4(51, struct.pack(">I", lease)) + opt4(1, b"\xff\xff\xff\x00") +
                 opt4(3, server) + END, op=2, yiaddr=yiaddr, siaddr=server, sname=b"dhcp.example", file=b"pxelinux.0")


def opt6(code, data=b"", length=None):
    return struct.pack(">HH", code, len(data) if length is None else length) + data


def dhcp6(options=b"", typ=1, txid=0x1a2b3c):
    return bytes([typ]) + txid.to_bytes(3, "big") + options


def solicit():
    """A Solicit with five options."""
    return dhcp6(opt6(1, DUID) + opt6(6, b"\x00\x17\x00\x18") + opt6(8, b"\x00\x00") + opt6(14) +
                 opt6(3, struct.pack(">III", 0x0027fe8f, 0, 0)))


def relay6(options=b"", typ=12, hops=1, link=LINK, peer=PEER):
    return bytes([typ, hops]) + link + peer + options


def ntp(first=0x23, stratum=2, poll=6, precision=0xe9, delay=0x00000a8c, dispersion=0x0000123d, refid=0xc0a80001,
        ts=(0xe1b2c3d400000001, 0xe1b2c3d500000002, 0xe1b2c3d600000003, 0xe1b2c3d700000004), ext=b""):
    return struct.pack(">BBBBIII4Q", first, stratum, poll, precision, delay, dispersion, refid, *ts) + ext


def over4(msg, sport=68, dport=67):
    return eth(ip4(udp(msg, sport, dport), 17))


def over6(msg, sport=546, dport=547):
    return eth(ip6(udp(msg, sport, dport), 17), 0x86dd)


def over_ntp(msg, sport=50123, dport=123):
    return eth(ip4(udp(msg, sport, dport), 17))


def front(lt, body):
    """The message straight behind Ethernet, through the table edit."""
    return eth(body, ET_OF[lt])


def quirk_cases():
    c = []
    E = {}

    def add(name, pkt, **expect):
        c.append((name, pkt))
        if expect:
            E[name] = expect
    # ---- DHCPv4 (dhcpv4.go:126-184)
    add("dhcp4_239_bytes", over4(dhcp4()[:239]), cls=1, lt=LT_DHCP4, err=160, a0=239, status=1, hdr=HDR)
    add("dhcp4_1_byte", over4(b"\x01"), cls=1, lt=LT_DHCP4, err=160, a0=1, status=1)
    add("dhcp4_240_bytes_contents_unset", over4(dhcp4()), cls=0, lt=LT_DHCP4, len=240, contents=0, nentries=0,
        b=[1, 1, 6, 0], v0=0x3903f326, v1=0x8000 << 16)
    add("dhcp4_241_bytes_end", over4(dhcp4(END)), cls=0, lt=LT_DHCP4, len=241, contents=241, nentries=0)
    add("dhcp4_241_bytes_pad", over4(dhcp4(PAD)), cls=0, len=241, contents=241, nentries=1, entries=[(0, 0, HDR + 241)])
    add("dhcp4_hlen_16", over4(dhcp4(END, hlen=16, chaddr=bytes(range(16)))), cls=0, lt=LT_DHCP4, b=[1, 1, 16, 0])
    add("dhcp4_hlen_17", over4(dhcp4(END, hlen=17)), cls=1, lt=LT_DHCP4, err=161, a0=17, status=0)
    add("dhcp4_hlen_255_bad_magic", over4(dhcp4(END, hlen=255, magic=bytes(4))), cls=1, err=161, a0=255, status=0)
    add("dhcp4_bad_magic", over4(dhcp4(END, magic=bytes.fromhex("63825362"))), cls=1, lt=LT_DHCP4, err=162, status=0)
    add("dhcp4_bad_magic_240", over4(dhcp4(magic=bytes(4))), cls=1, err=162, status=0)
    add("dhcp4_discover_eight_options", over4(discover()), cls=0, lt=LT_DHCP4, nentries=8, contents=len(discover()),
        entries=[(53, 1, HDR + 242), (61, 7, HDR + 245), (12, 6, HDR + 254), (60, 8, HDR + 262), (50, 4, HDR + 272),
                 (55, 13, HDR + 278), (57, 2, HDR + 293), (51, 4, HDR + 297)])
    add("dhcp4_ack", over4(ack(), 67, 68), cls=0, lt=LT_DHCP4, nentries=5, b=[2, 1, 6, 0],
        v2=0, v3=int.from_bytes(bytes([10, 0, 0, 99]), "little"), v4=int.from_bytes(bytes([10, 0, 0, 1]), "little"), v5=0)
    add("dhcp4_option_ends_at_the_end", over4(dhcp4(opt4(53, b"\x03") + opt4(12, b"abc"))), cls=0, nentries=2,
        entries=[(53, 1, HDR + 242), (12, 3, HDR + 245)], contents=248)
    add("dhcp4_lone_type_byte", over4(dhcp4(opt4(53, b"\x03") + b"\x0c")), cls=1, lt=LT_DHCP4, err=163, status=0,
        nentries=0)
    add("dhcp4_length_one_past_the_end", over4(dhcp4(opt4(12, b"abc", length=4))), cls=1, err=164, status=0)
    add("dhcp4_length_255_two_bytes", over4(dhcp4(b"\x0c\xff")), cls=1, err=164, status=0)
    add("dhcp4_zero_length_option_at_the_end", over4(dhcp4(opt4(80))), cls=0, nentries=1, entries=[(80, 0, HDR + 242)])
    add("dhcp4_pad_run", over4(dhcp4(PAD * 5 + opt4(53, b"\x01") + PAD * 2 + END)), cls=0, nentries=8,
        entries=[(0, 0, HDR + 241 + k) for k in range(5)] + [(53, 1, HDR + 247), (0, 0, HDR + 249), (0, 0, HDR + 250)])
    add("dhcp4_end_then_garbage", over4(dhcp4(opt4(53, b"\x02") + END + b"\x0c\xff garbage")), cls=0, nentries=1,
        contents=240 + 3 + 1 + 10, entries=[(53, 1, HDR + 242)])
    add("dhcp4_no_end", over4(dhcp4(opt4(53, b"\x01") + opt4(12, b"x"))), cls=0, nentries=2)
    add("dhcp4_end_first_then_lone_byte", over4(dhcp4(END + b"\x0c")), cls=0, nentries=0, contents=242)
    add("dhcp4_300_pads", over4(dhcp4(PAD * 300)), cls=0, nentries=300, len=540)
    # ---- DHCPv6 (dhcpv6.go:89-124, dhcpv6_options.go:611-622)
    add("dhcp6_3_bytes", over6(dhcp6()[:3]), cls=1, lt=LT_DHCP6, err=165, a0=3, status=1, hdr=HDR6)
    add("dhcp6_4_bytes", over6(dhcp6()), cls=0, lt=LT_DHCP6, len=4, contents=4, nentries=0, b=[1, 0, 0, 0], v0=0x1a2b3c,
        v1=0, v2=0)
    add("dhcp6_7_bytes", over6(dhcp6(b"\x00\x01\x00")), cls=1, lt=LT_DHCP6, err=167, status=0)
    add("dhcp6_solicit_five_options", over6(solicit()), cls=0, lt=LT_DHCP6, nentries=5, contents=len(solicit()),
        entries=[(1, 14, HDR6 + 8), (6, 4, HDR6 + 26), (8, 2, HDR6 + 34), (14, 0, HDR6 + 40), (3, 12, HDR6 + 44)])
    add("dhcp6_relay_33_bytes", over6(relay6()[:33], 547, 547), cls=1, lt=LT_DHCP6, err=166, a0=33, a1=12, status=1)
    add("dhcp6_relay_reply_5_bytes", over6(relay6(typ=13)[:5], 547, 547), cls=1, err=166, a0=5, a1=13, status=1)
    add("dhcp6_relay_34_bytes", over6(relay6(), 547, 547), cls=0, lt=LT_DHCP6, len=34, nentries=0, b=[12, 1, 0, 0], v0=0,
        v1=HDR6 + 2, v2=HDR6 + 18)
    add("dhcp6_relay_with_message", over6(relay6(opt6(9, solicit()) + opt6(18, b"eth0"), typ=12, hops=3), 547, 547),
        cls=0, nentries=2, b=[12, 3, 0, 0], entries=[(9, len(solicit()), HDR6 + 38), (18, 4, HDR6 + 38 + len(solicit()) + 4)])
    add("dhcp6_type_12_is_relay_even_at_4_bytes", over6(bytes([12, 0, 0, 0])), cls=1, err=166, a0=4, a1=12, status=1)
    add("dhcp6_option_length_fffe", over6(dhcp6(opt6(1, b"abcd", length=0xfffe))), cls=1, lt=LT_DHCP6, err=168, a0=2,
        status=0)
    add("dhcp6_option_length_fffb", over6(dhcp6(opt6(1, b"abcd", length=0xfffb))), cls=1, err=168, a0=0xffff, status=0)
    add("dhcp6_option_length_fffc", over6(dhcp6(opt6(1, b"", length=0xfffc))), cls=1, err=168, a0=0, status=0)
    add("dhcp6_option_one_past_the_end", over6(dhcp6(opt6(1, DUID) + opt6(8, b"\x00", length=2))), cls=1, err=168, a0=6,
        status=0)
    add("dhcp6_option_ends_at_the_end", over6(dhcp6(opt6(1, DUID) + opt6(8, b"\x00\x07"))), cls=0, nentries=2,
        entries=[(1, 14, HDR6 + 8), (8, 2, HDR6 + 26)])
    add("dhcp6_reply_from_server", over6(dhcp6(opt6(2, DUID) + opt6(1, DUID) + opt6(7, b"\xff"), typ=7), 547, 546), cls=0,
        b=[7, 0, 0, 0], nentries=3)
    # the one unguarded slice: Length 0xFFFD with 65 537 bytes behind the option's head (an EtherType edit's payload)
    add("dhcp6_option_length_fffd_fits_panics", front(LT_DHCP6, dhcp6(opt6(1, bytes(0xfffd)))), cls=1, lt=LT_DHCP6, err=4,
        a0=4, a1=1, status=0, hdr=14)
    add("dhcp6_option_length_fffb_fits", front(LT_DHCP6, dhcp6(opt6(1, bytes(0xfffb)))), cls=0, nentries=1,
        entries=[(1, 0xfffb, 14 + 8)])
    # ---- NTP (ntp.go:294-347)
    add("ntp_47_bytes", over_ntp(ntp()[:47]), cls=1, lt=LT_NTP, err=169, status=1, hdr=HDR)
    add("ntp_48_bytes", over_ntp(ntp()), cls=0, lt=LT_NTP, len=48, contents=48, nentries=0, b=[0, 4, 3, 2],
        v0=6 | 0xe9 << 8, v1=0xa8c, v2=0x123d, v3=0xc0a80001, v4=HDR + 48, v5=0)
    add("ntp_60_bytes_extension", over_ntp(ntp(0xdc, 1, ext=b"extension!!!")), cls=0, lt=LT_NTP, len=60, contents=60,
        b=[3, 3, 4, 1], v4=HDR + 48, v5=12)
    add("ntp_server_reply", over_ntp(ntp(0x24, 1, refid=0x47505300), 123, 50123), cls=0, b=[0, 4, 4, 1], v3=0x47505300)
    # ---- the ways to a message
    add("by_source_port_alone", over_ntp(ntp(), 123, 50000), cls=0, lt=LT_NTP)
    add("dhcp4_by_source_port_68", over4(discover(), 68, 50000), cls=0, lt=LT_DHCP4)
    add("destination_port_wins", over4(ntp(), 67, 123), cls=0, lt=LT_NTP)       # dport 123 before sport 67
    add("destination_port_wins_and_fails", over4(discover()[:100], 123, 67), cls=1, lt=LT_DHCP4, err=160, a0=100)
    add("registered_udp_port_dhcp4", over4(discover(), 50001, 9067), cls=0, lt=LT_DHCP4, nentries=8)
    add("registered_udp_port_dhcp6", over6(solicit(), 50001, 9546), cls=0, lt=LT_DHCP6, nentries=5)
    add("registered_udp_port_ntp", over_ntp(ntp(), 9123, 50001), cls=0, lt=LT_NTP)
    add("registered_tcp_port_dhcp4", eth(ip4(tcp(ack(), dport=8067), 6)), cls=0, lt=LT_DHCP4, hdr=14 + 20 + 20, nentries=5)
    add("ethertype_edit_ntp", front(LT_NTP, ntp()), cls=0, lt=LT_NTP, hdr=14)
    add("ethertype_edit_dhcp4_short", front(LT_DHCP4, dhcp4()[:200]), cls=1, lt=LT_DHCP4, err=160, a0=200, hdr=14)
    add("dhcp6_over_ipv4", over4(solicit(), 546, 547), cls=0, lt=LT_DHCP6, hdr=HDR)
    add("dhcp4_over_ipv6", over6(discover(), 68, 67), cls=0, lt=LT_DHCP4, hdr=HDR6)
    add("behind_vxlan_dhcp4", over_udp(vxlan(over4(ack(), 67, 68)), VX))       # the outer level: no candidate
    # ---- not candidates
    add("udp_empty_payload_port_67", over4(b"", 68, 67))
    add("plain_udp", eth(ip4(udp(bytes(12), 50004, 50005), 17)))
    add("dns_query_port_53", eth(ip4(udp(bytes(12), 50004, 53), 17)))
    add("tcp_port_123_is_not_ntp", eth(ip4(tcp(ntp(), dport=123), 6)))
    add("ns_behind_icmp6", NC.behind(NC.LT_NS, NC.ns(NC.opt_lladdr())))
    return c, E


def layers17():
    """Ethernet, 13 Dot1Q tags, IPv4, UDP: 16 layers in front of the message; and one tag more (UNKNOWN)."""
    tags = lambda n: MAC + b"".join(b"\x81\x00" + b"\x00\x05" for _ in range(n)) + b"\x08\x00"  # noqa: E731
    return tags(13) + ip4(udp(ntp(), 50123, 123), 17), tags(14) + ip4(udp(ntp(), 50123, 123), 17)


def bodies(rnd):
    """One well-formed message of a random layer: (layer type, body)."""
    lt = rnd.choice(LAYER_TYPES)
    blob = lambda n: bytes(rnd.randrange(256) for _ in range(n))  # noqa: E731
    if lt == LT_DHCP4:
        opts = b"".join(rnd.choice([lambda: opt4(53, bytes([rnd.randrange(1, 9)])), lambda: opt4(12, b"host-%d" % rnd.randrange(99)),
                                    lambda: opt4(rnd.randrange(1, 255), blob(rnd.randrange(0, 20))), lambda: PAD,
                                    lambda: opt4(51, blob(4)), lambda: opt4(54, blob(4))])()
                        for _ in range(rnd.choice([0, 1, 2, 3, 5, 8])))
        tail = rnd.choice([END, END, END + blob(rnd.randrange(1, 6)), b""])
        return lt, dhcp4(opts + tail, op=rnd.choice([1, 2]), hlen=rnd.choice([6, 6, 6, 0, 16]), xid=rnd.randrange(1 << 32),
                         yiaddr=blob(4), chaddr=blob(6))
    if lt == LT_DHCP6:
        opts = b"".join(rnd.choice([lambda: opt6(1, DUID), lambda: opt6(rnd.randrange(1, 144), blob(rnd.randrange(0, 24))),
                                    lambda: opt6(14), lambda: opt6(8, blob(2))])() for _ in range(rnd.choice([0, 1, 2, 3, 5])))
        if rnd.random() < 0.3:
            return lt, relay6(opts, rnd.choice([12, 13]), rnd.randrange(32))
        return lt, dhcp6(opts, rnd.randrange(1, 12), rnd.randrange(1 << 24))
    return lt, ntp(rnd.randrange(256), rnd.randrange(17), rnd.randrange(256), rnd.randrange(256), rnd.randrange(1 << 32),
                   ext=blob(rnd.choice([0, 0, 0, 4, 20])))


PORTS = {LT_DHCP4: (68, 67), LT_DHCP6: (546, 547), LT_NTP: (50123, 123)}
BIG = 4096  # the cases longer than this are mixed in as they are only


def corpus(seed, n, vectors=()):
    """The cases and the vectors as they are (first), then these with bytes
    changed or cut short, and generated messages of every layer, whole, with a
    length or type byte changed, or cut near the end. `vectors`: packets
    (bytes) to mix in."""
    rnd = random.Random(seed)
    base = [p for _, p in quirk_cases()[0]] + list(vectors)
    out = list(base)
    small = [p for p in base if len(p) <= BIG]
    while len(out) < n:
        r = rnd.random()
        if r < 0.25:
            pkt = bytearray(rnd.choice(small))
            how = rnd.random()
            if how < 0.4 and len(pkt) > 44:
                for _ in range(rnd.randrange(1, 3)):
                    pkt[rnd.randrange(42, len(pkt))] = rnd.randrange(256)
            elif how < 0.7:
                pkt = pkt[:rnd.randrange(max(1, len(pkt) - 24), len(pkt) + 1)]
            out.append(bytes(pkt))
            continue
        lt, body = bodies(rnd)
        body = bytearray(body)
        how = rnd.random()
        if how < 0.3:        # a byte of the option area (or of the head) changed: lengths and types included
            lo = {LT_DHCP4: 236, LT_DHCP6: 0, LT_NTP: 0}[lt] if rnd.random() < 0.8 else 0
            if len(body) > lo:
                body[rnd.randrange(lo, len(body))] = rnd.choice([0, 1, 2, 255, 12, 13, rnd.randrange(256)])
        elif how < 0.55:     # cut near its end or near its fixed part
            body = body[:rnd.choice([rnd.randrange(0, len(body) + 1), max(0, len(body) - rnd.randrange(1, 12)),
                                     rnd.randrange(0, 50), rnd.randrange(236, 246)])]
        elif how < 0.6:      # bytes added behind it
            body += bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 9)))
        body = bytes(body)
        sport, dport = PORTS[lt]
        w = rnd.random()
        if w < 0.15:
            out.append(front(lt, body))
        elif w < 0.3:
            out.append(eth(ip6(udp(body, sport, dport), 17), 0x86dd))
        elif w < 0.4:
            out.append(eth(ip4(udp(body, dport, sport), 17)))
        else:
            out.append(eth(ip4(udp(body, sport, dport), 17)))
    return out[:n]


CORPUS_SEED = 20261021
CORPUS_N = 2048
