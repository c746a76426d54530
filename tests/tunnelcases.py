"""Hand-derived tunnel packets, one per quirk of include/gpk_tunnel.h (items 4-7
of DESIGN.md §19), and the seeded fuzz corpus of the tunnel tests.

Every case is (name, packet bytes). The expected values come from
tunnel_model.py; the cases that pin a quirk also carry the expected outcome by
hand in EXPECT (tunnel error code and arguments, or contents / inner length),
derived from the reference's source, so the model is checked too.
"""
import random
import struct

PARSER = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"])
PARSER_IGNORE = dict(PARSER, ignore_unsupported=True)
MAC = bytes.fromhex("0242ac110002" "0242ac110003")


def eth(payload, et=0x0800):
    return MAC + struct.pack(">H", et) + payload


def dot1q(payload, et=0x0800, vid=5):
    return struct.pack(">HH", vid, et) + payload


def ip4(payload, proto, total=None, src=b"\x0a\x00\x00\x01", dst=b"\x0a\x00\x00\x02"):
    total = 20 + len(payload) if total is None else total
    return struct.pack(">BBHHHBBH", 0x45, 0, total & 0xffff, 1, 0, 64, proto, 0) + src + dst + payload


def ip6(payload, nh, plen=None):
    plen = len(payload) if plen is None else plen
    return struct.pack(">IHBB", 6 << 28, plen, nh, 64) + bytes(15) + b"\x01" + bytes(15) + b"\x02" + payload


def udp(payload, sport, dport, length=None):
    length = 8 + len(payload) if length is None else length
    return struct.pack(">HHHH", sport, dport, length, 0) + payload


def tcp(payload, sport=40000, dport=80):
    return struct.pack(">HHIIBBHHH", sport, dport, 1, 2, 0x50, 0x18, 1000, 0, 0) + payload


def inner_eth(n=20):
    return eth(ip4(tcp(bytes(range(n))), 6))


def vxlan(inner, b0=0x08, b1=0, gbp=0, vni=0x123456, rsv=0):
    return bytes([b0, b1]) + struct.pack(">H", gbp) + vni.to_bytes(3, "big") + bytes([rsv]) + inner


def geneve(inner, proto=0x6558, opts=b"", optlen=None, ver=0, b1=0, vni=0xabcdef):
    optlen = len(opts) // 4 if optlen is None else optlen
    return bytes([ver << 6 | (optlen & 0x3f), b1]) + struct.pack(">H", proto) + vni.to_bytes(3, "big") + b"\x00" + \
        opts + inner


def gopt(data_words=0, cls=0x0102, typ=0x80, flags=0):
    return struct.pack(">HBB", cls, typ, flags << 5 | data_words) + bytes(range(4 * data_words))


def gre(inner, proto=0x0800, b0=0, b1=0, csum=0, off=0, key=None, seq=None, sres=None, ack=None):
    """b0 / b1 extra flag bits; fields given set their flag."""
    h = b""
    if b0 & 0xC0:
        h += struct.pack(">HH", csum, off)
    if key is not None:
        b0 |= 0x20
        h += struct.pack(">I", key)
    if seq is not None:
        b0 |= 0x10
        h += struct.pack(">I", seq)
    if sres is not None:
        assert b0 & 0x40
        for af, so, info in sres:
            h += struct.pack(">HBB", af, so, len(info)) + info
        h += bytes(4)
    if ack is not None:
        b1 |= 0x80
        h += struct.pack(">I", ack)
    return bytes([b0, b1]) + struct.pack(">H", proto) + h + inner


def gre_with_checksum(inner, proto=0x0800, good=True, **kw):
    """A GRE header with the C bit whose checksum field makes the sum fold to it."""
    body = gre(inner, proto, b0=0x80, csum=0, **kw)
    s = 0
    for i in range(0, len(body) - 1, 2):
        s += body[i] << 8 | body[i + 1]
    if len(body) & 1:
        s += body[-1] << 8
    while s > 0xffff:
        s = (s >> 16) + (s & 0xffff)
    c = ~s & 0xffff
    if not good:
        c ^= 0x0100
    return body[:4] + struct.pack(">H", c) + body[6:]


def over_udp(tun, dport, pad=0, declared=None):
    """Ethernet / IPv4 / UDP around a tunnel header. declared: the tunnel
    bytes the UDP and IPv4 length fields announce (default all); pad: bytes
    after the IPv4 datagram (Ethernet padding: they count for cap, not len)."""
    d = len(tun) if declared is None else declared
    return eth(ip4(udp(tun, 50000, dport, 8 + d), 17, 28 + d)) + bytes(pad)


def over_ip(tun, pad=0, declared=None, v6=False):
    d = len(tun) if declared is None else declared
    if v6:
        return eth(ip6(tun, 47, d), 0x86dd) + bytes(pad)
    return eth(ip4(tun, 47, 20 + d)) + bytes(pad)


VX, GN = 4789, 6081


def quirk_cases():
    c = []
    E = {}

    def add(name, pkt, **expect):
        c.append((name, pkt))
        if expect:
            E[name] = expect
    ie = inner_eth()
    # ---- VXLAN (vxlan.go:53-78)
    add("vxlan_plain", over_udp(vxlan(ie), VX), contents=8, inner=len(ie), next=17)
    add("vxlan_len7", over_udp(vxlan(b"")[:7], VX), err=70, trunc=0)
    add("vxlan_len8_empty_payload", over_udp(vxlan(b""), VX), contents=8, inner=0, next=17, cls=4)
    add("vxlan_I_clear_gbp", over_udp(vxlan(ie, b0=0x80, b1=0xC0, gbp=0x1234), VX), contents=8, inner=len(ie), bits=2 | 4 | 8)
    add("vxlan_short_inner", over_udp(vxlan(ie[:9]), VX), contents=8, inner=9)
    # ---- Geneve (geneve.go:59-119)
    add("geneve_plain", over_udp(geneve(ie), GN), contents=8, inner=len(ie), next=17)
    add("geneve_len6", over_udp(geneve(b"")[:6], GN), err=75, trunc=1)
    add("geneve_len7_cap7", over_udp(geneve(b"")[:7], GN), err=3, a0=8, a1=7)          # data[:8], cap 7
    add("geneve_len7_cap10", over_udp(geneve(b"") + b"\xee", GN, declared=7, pad=1), err=4, a0=8, a1=7)  # data[8:]
    add("geneve_len8", over_udp(geneve(b""), GN), contents=8, inner=0, cls=4)
    add("geneve_opts_short", over_udp(geneve(b"", optlen=2)[:14], GN), err=76, trunc=1)   # 14 < 8 + 7
    add("geneve_opt_3_left", over_udp(geneve(b"\x01\x02\x80", optlen=1), GN), err=2, a0=3, a1=3)  # len == OptLen + 7
    add("geneve_declared_10_of_11", over_udp(geneve(b"\x01\x02" + bytes(6), optlen=1), GN, declared=10), err=76, trunc=1)
    add("geneve_opt_len_exceeds", over_udp(geneve(gopt(0)[:3] + b"\x02" + bytes(4), optlen=1), GN), err=74, trunc=1)
    # an option longer than the declared OptionsLength: the walk overshoots, length goes negative
    add("geneve_opt_overruns_declared", over_udp(geneve(gopt(3) + ie, optlen=1), GN), contents=24, count=1)
    add("geneve_two_options", over_udp(geneve(ie, opts=gopt(1) + gopt(0)), GN), contents=20, count=2, inner=len(ie))
    # options summing to 248: offset 8 + 248 = 256 wraps to 0; with OptionsLength 252 the walk goes on at data[0:]
    o248 = gopt(31) + gopt(29)
    assert len(o248) == 248
    add("geneve_opts_248", over_udp(geneve(ie, opts=o248), GN), contents=0, count=2, inner=8 + 248 + len(ie))
    # ... and then reads an "option" at the header's own bytes: data[3] = 0x58 gives Length 100
    add("geneve_opts_248_plus_4", over_udp(geneve(ie, opts=o248 + gopt(0)), GN), contents=100, count=3)
    # the declared maximum alone: 8 + 252 = 260 wraps to 4
    add("geneve_opts_252", over_udp(geneve(ie, opts=gopt(31) + gopt(30)), GN), contents=4, count=2,
        inner=4 + 252 + len(ie))
    add("geneve_version_bit", over_udp(geneve(ie, ver=2, b1=0xC0), GN), version=1, bits=3)
    add("geneve_version_1_reads_0", over_udp(geneve(ie, ver=1), GN), version=0, optlen=0)  # bit 6 is read by nothing
    add("geneve_ipv4", over_udp(geneve(ie[14:], proto=0x0800), GN), next=20, cls=2)
    add("geneve_ipv6", over_udp(geneve(ip6(tcp(b"hello"), 6), proto=0x86dd), GN), next=21, cls=3)
    add("geneve_dot1q", over_udp(geneve(dot1q(ie[14:]), proto=0x8100), GN), next=15, cls=1)
    add("geneve_unknown_proto", over_udp(geneve(ie, proto=0x1234), GN), next=0, cls=4)
    add("geneve_unregistered", over_udp(geneve(ie, proto=0x0806), GN), next=10, cls=4)  # ARP: no decoder
    # ---- GRE (gre.go:40-128)
    i4 = ie[14:]
    add("gre_plain", over_ip(gre(i4)), contents=4, inner=len(i4), next=20, cls=2)
    add("gre_len3", over_ip(gre(b"")[:3]), err=71, trunc=1)
    add("gre_len4_empty", over_ip(gre(b"")), contents=4, inner=0, cls=4)
    add("gre_teb", over_ip(gre(ie, 0x6558)), next=17, cls=0)
    add("gre_ipv6", over_ip(gre(ip6(tcp(b"x"), 6), 0x86dd), v6=True), next=21, cls=3)
    add("gre_dot1q_88a8", over_ip(gre(dot1q(i4), 0x88a8)), next=15, cls=1)
    add("gre_C", over_ip(gre(i4, b0=0x80, csum=0x1111, off=0x2222)), contents=8, csum=0x1111, off=0x2222)
    add("gre_R_word_without_C", over_ip(gre(i4, b0=0x40, csum=0x3333, off=4, sres=[])), contents=12, csum=0x3333, count=0)
    add("gre_C_R", over_ip(gre(i4, b0=0xC0, csum=1, off=2, sres=[(2, 0, b"\x0a\x00\x00\x09")])), contents=20, count=1)
    add("gre_R_3_sres", over_ip(gre(i4, b0=0x40, sres=[(2, 0, b"abcd"), (2, 4, b"efghijkl"), (7, 0, b"")])),
        contents=8 + 8 + 12 + 4 + 4, count=3)
    add("gre_C_word_missing", over_ip(gre(b"", b0=0x80)[:6]), err=72, trunc=1)
    add("gre_key_seq_ack", over_ip(gre(i4, key=0xdeadbeef, seq=7, ack=9)), contents=16, key=0xdeadbeef, seq=7, ack=9)
    add("gre_seq_missing", over_ip(gre(b"", key=1, seq=2)[:10]), err=72, trunc=1)
    add("gre_ack_missing", over_ip(gre(b"", ack=2)[:7]), err=72, trunc=1)
    add("gre_null_sre_cut", over_ip(gre(b"", b0=0x40, sres=[(2, 0, b"abcd")])[:18]), err=72, trunc=1)
    add("gre_sre_overruns", over_ip(gre(b"", b0=0x40, sres=[(2, 0, b"abcdefgh")])[:14]), err=72, trunc=1)
    add("gre_af0_len4_listed", over_ip(gre(i4, b0=0x40, sres=[(0, 0, b"abcd")])), count=1)
    add("gre_version_1_pptp", over_ip(gre(i4, 0x880b, b1=1, key=5)), cls=4)  # PPP: no decoder
    add("gre_checksum_good", over_ip(gre_with_checksum(i4)), status=2 | 4)
    add("gre_checksum_bad", over_ip(gre_with_checksum(i4, good=False)), status=2)
    add("gre_checksum_odd_len", over_ip(gre_with_checksum(i4 + b"\x7f")), status=2 | 4)
    # ---- nesting and plain traffic
    add("vxlan_in_gre", over_ip(gre(ip4(udp(vxlan(ie), 50001, VX), 17))))
    add("geneve_in_geneve", over_udp(geneve(eth(ip4(udp(geneve(ie), 50002, GN), 17))), GN))
    add("gre_over_ip6_geneve_ip6_udp", over_ip(gre(ip6(udp(geneve(eth(ip6(udp(b"dns?", 5353, 53), 17), 0x86dd),
                                                                  opts=gopt(2)), 50003, GN), 17), 0x86dd), v6=True))
    add("plain_tcp", ie)
    add("plain_udp_dns", eth(ip4(udp(bytes(12), 50004, 53), 17)))
    add("vxlan_dot1q_outer", MAC + struct.pack(">H", 0x8100) + dot1q(ip4(udp(vxlan(ie), 50005, VX), 17)))
    add("vxlan_empty_udp", eth(ip4(udp(b"", 50006, VX), 17)))  # empty payload: not a candidate
    return c, E


def fuzz_packets(seed, n):
    """Valid encapsulations with one to three mutated tunnel-header bytes and
    random truncation, aimed at the header's own length boundaries."""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        k = rnd.randrange(10)
        inner = rnd.choice([inner_eth(rnd.randrange(0, 40)), inner_eth()[14:], ip6(tcp(b"six"), 6), dot1q(inner_eth()[14:]),
                            b"", bytes(rnd.randrange(1, 12))])
        if k < 3:
            tun = vxlan(inner if rnd.random() < 0.8 else b"", b0=rnd.choice([0x08, 0x88, 0]), vni=rnd.randrange(1 << 24))
            hdr, wrap = 8, lambda t, **kw: over_udp(t, VX, **kw)
        elif k < 6:
            opts = b"".join(gopt(rnd.choice([0, 0, 1, 2, 31])) for _ in range(rnd.choice([0, 0, 1, 2, 3])))[:252]
            proto = rnd.choice([0x6558, 0x0800, 0x86dd, 0x8100, 0x0806, 0x1234])
            tun = geneve(inner, proto=proto, opts=opts, ver=rnd.choice([0, 0, 2]), b1=rnd.choice([0, 0x80, 0x40]))
            hdr, wrap = 8 + len(opts), lambda t, **kw: over_udp(t, GN, **kw)
        else:
            kw = {}
            b0 = rnd.choice([0, 0, 0x80, 0x40, 0xC0])
            if rnd.random() < 0.4:
                kw["key"] = rnd.randrange(1 << 32)
            if rnd.random() < 0.3:
                kw["seq"] = rnd.randrange(1 << 32)
            if rnd.random() < 0.2:
                kw["ack"] = rnd.randrange(1 << 32)
            if b0 & 0x40:
                kw["sres"] = [(rnd.choice([0, 2]), 0, bytes(rnd.choice([0, 4, 8]))) for _ in range(rnd.randrange(3))]
            proto = rnd.choice([0x6558, 0x0800, 0x86dd, 0x8100, 0x88a8, 0x880b, 0x4321])
            if b0 & 0x80 and rnd.random() < 0.7:
                tun = gre_with_checksum(inner, proto, good=rnd.random() < 0.7, **{x: kw[x] for x in kw if x != "sres"})
            else:
                tun = gre(inner, proto, b0=b0, csum=rnd.randrange(1 << 16), **kw)
            hdr = len(tun) - len(inner)
            v6 = rnd.random() < 0.3
            wrap = lambda t, v6=v6, **kw: over_ip(t, v6=v6, **kw)  # noqa: E731
        tun = bytearray(tun)
        if rnd.random() < 0.6:  # mutate header bytes
            for _ in range(rnd.randrange(1, 4)):
                if len(tun):
                    tun[rnd.randrange(min(len(tun), max(hdr, 4)))] = rnd.randrange(256)
        tun = bytes(tun)
        r = rnd.random()
        if r < 0.25:    # the lengths declare only part of the tunnel bytes; the rest is padding (cap > len)
            pkt = wrap(tun, declared=rnd.randrange(0, min(len(tun), hdr + 6) + 1))
        elif r < 0.5:   # cut near the header's end
            cut = rnd.randrange(0, min(len(tun), hdr + 6) + 1)
            pkt = wrap(tun[:cut])
        elif r < 0.6:   # cut anywhere in the whole packet
            pkt = wrap(tun)
            pkt = pkt[:rnd.randrange(1, len(pkt) + 1)]
        else:
            pkt = wrap(tun)
        out.append(pkt)
    return out


FUZZ_SEED = 20261020
FUZZ_N = 4096
