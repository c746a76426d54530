"""The packets of tests/test_serialize_*.py: the smallest shapes at which
gpk_serialize_batch can go wrong (include/gpk_serialize.h), decoded by the CPU
oracle for their layouts and fields records, then edited by name.

build() -> dict(data, offsets, caplens, layouts, fields, names): one batch, all
first layer Ethernet. Every case is small except the few whose point is a size
(65 535 / 70 000 bytes, the 262 144 bytes of 0xff whose sum wraps mod 2^32).

Alignments. The mover's paths depend on the output address (the byte head up
to the first 16-byte store), on the shift between source and output address,
and on the length (vectors, byte tail). For every tail length 0..70 and
1440..1480 there are 16 packets: their source alignments sweep 0..15 (padding in
the data buffer) and their output offsets sweep 0..15 (a short undecodable
filler packet in front, which serializes to its own bytes), paired with a
rotation that depends on the length, so that over the lengths every (source,
output) pair occurs several times. A full 16 x 16 product per length would be
28 672 packets and checks no further path.

What a decoded layout cannot reach: more than 65 535 bytes behind an IPv4 or
IPv6 header that has a transport layer (both decodes trim their payload to a
16-bit length; an IPv6 jumbogram leaves its HopByHop in the payload,
ip6.go:249-256, so no transport layer decodes inside one). The FixLengths wrap
of IPv4.Length, UDP's jumbo Length, "Cannot fit payload length of %d into IPv6
packet" and a sum that wraps mod 2^32 are therefore reached with a layout the
caller widened ("wide": the transport slice runs to the end of the packet, as
a caller that reassembled a TSO burst would hand it over; "jumbo_udp": the IPv6
and UDP slices of a UDP jumbogram with its HopByHop in place).
"""
import struct

import numpy as np

from gopacket_amd import _lib
from oracle import oracle as O

DECODERS = ["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"]
ETH, D1Q, IP4, IP6, EXT, TCP, UDP, PAY = range(8)
MAC_A, MAC_B = bytes.fromhex("020000000001"), bytes.fromhex("0200000000fe")


def csum16(b):
    if len(b) & 1:
        b += b"\0"
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def eth(payload, etype, dst=MAC_B, src=MAC_A):
    return dst + src + struct.pack(">H", etype) + payload


def vlan(payload, etype, tci=0x6064):
    return struct.pack(">HH", tci, etype) + payload


def ip4(payload, proto, opts=b"", length=None, src=bytes([10, 1, 2, 3]), dst=bytes([192, 168, 7, 9]), ttl=64, frag=0x4000):
    ihl = 5 + len(opts) // 4
    total = 20 + len(opts) + len(payload) if length is None else length
    h = bytearray(struct.pack(">BBHHHBBH", 0x40 | ihl, 0x10, total & 0xFFFF, 0x1234, frag, ttl, proto, 0) + src + dst + opts)
    h[10:12] = struct.pack(">H", csum16(bytes(h)))
    return bytes(h) + payload


IP6_A = bytes.fromhex("20010db8000000000000000000000001")
IP6_B = bytes.fromhex("20010db800000000000000000000beef")


def ip6(payload, nh, length=None, src=IP6_A, dst=IP6_B):
    ln = len(payload) if length is None else length
    return struct.pack(">IHBB", 0x6A5B1234 & 0x6FFFFFFF, ln & 0xFFFF, nh, 63) + src + dst + payload


def tcp(payload, opts=b"", pseudo=None, sport=443, dport=51000):
    doff = 5 + len(opts) // 4
    h = bytearray(struct.pack(">HHIIHHHH", sport, dport, 0x01020304, 0xA0B0C0D0, doff << 12 | 0x018, 0x7210, 0, 0) + opts)
    if pseudo is not None:
        n = len(h) + len(payload)
        h[16:18] = struct.pack(">H", csum16(pseudo + struct.pack(">HH", 6, n) + bytes(h) + payload))
    return bytes(h) + payload


def udp(payload, length=None, pseudo=None, sport=5353, dport=4000):
    ln = 8 + len(payload) if length is None else length
    h = bytearray(struct.pack(">HHHH", sport, dport, ln & 0xFFFF, 0))
    if pseudo is not None:
        c = csum16(pseudo + struct.pack(">HH", 17, ln) + bytes(h) + payload)
        h[6:8] = struct.pack(">H", c or 0xFFFF)
    return bytes(h) + payload


def blob(n, seed=1):
    return np.random.default_rng(seed * 7919 + n).integers(0, 256, n, dtype=np.uint8).tobytes()


P4 = bytes([10, 1, 2, 3]) + bytes([192, 168, 7, 9])


def tcp4(n, seed=1, opts=b"", ip_opts=b""):
    pl = blob(n, seed)
    return eth(ip4(tcp(pl, opts, pseudo=P4), 6, ip_opts), 0x0800)


def udp4(n, seed=1):
    return eth(ip4(udp(blob(n, seed), pseudo=P4), 17), 0x0800)


def udp6(n, seed=1):
    return eth(ip6(udp(blob(n, seed), pseudo=IP6_A + IP6_B), 17), 0x86DD)


def hbh(nh, opts):
    assert (2 + len(opts)) % 8 == 0
    return bytes([nh, (2 + len(opts)) // 8 - 1]) + opts


def jumbo6(n, value=None):
    body = hbh(59, bytes([0xC2, 4]) + struct.pack(">I", 8 + n if value is None else value)) + blob(n, 5)
    return eth(ip6(body, 0, length=0), 0x86DD)


# ---- edits of the fields record, by name ------------------------------------
def _clear(bit):
    def f(r):
        r["present"] &= 0xFF ^ (1 << bit)
    return f


def _set(**kv):
    def f(r):
        for k, v in kv.items():
            r[k] = v
    return f


def _vlan_pop(r):
    r["present"] &= 0xFF ^ (1 << D1Q)
    r["eth_type"] = r["d1q_type"]


def _setbit(bit):
    def f(r):
        r["present"] |= 1 << bit
    return f


def _drop_hbh_options(r):
    r["hbh_opt_map"] = 0


def cases():
    """[(name, packet bytes, edit or None)]"""
    c = []
    # Ethernet pad on each side of 60: frames of 14..61 bytes
    for n in range(14, 62):
        if n >= 54:
            c.append(("pad_tcp_%d" % n, tcp4(n - 54, n), None))
        elif n >= 42:
            c.append(("pad_udp_%d" % n, udp4(n - 42, n), None))
        elif n >= 34:
            c.append(("pad_ip4_%d" % n, eth(ip4(blob(n - 34, n), 253), 0x0800), None))
        else:
            c.append(("pad_eth_%d" % n, eth(blob(n - 14, n), 0x88B5), None))
    c.append(("eth_trailer", tcp4(3) + b"\xEE" * 9, None))  # the trailer is dropped, then the pad
    # sizes: Length wraps (IPv4, TSO Length 0), the UDP Length, the IPv6 limits
    for n in (65535, 70000):
        c.append(("ip4_tso_tcp_%d" % n, eth(ip4(tcp(blob(n, 3), pseudo=None), 6, length=0), 0x0800), None))
        c.append(("ip4_tso_udp_%d" % n, eth(ip4(udp(blob(n, 4), length=0), 17, length=0), 0x0800), None))
        c.append(("ip6_jumbo_%d" % n, jumbo6(n), None))
        c.append(("ip6_jumbo_notlv_%d" % n, jumbo6(n), _drop_hbh_options))
    c.append(("ip6_udp_len0_max", eth(ip6(udp(blob(65527, 6), length=0), 17), 0x86DD), None))
    c.append(("ip6_max", eth(ip6(blob(65535, 7), 59), 0x86DD), None))
    # UDP's jumbo Length (udp.go:62-81): 70 000 bytes of UDP behind an IPv6 header whose inline HopByHop already
    # carries a 4-byte jumbo option. The reference's decode refuses a jumbo option next to a non-zero Length
    # (ip6.go:257-258), so the caller hands the IPv6 and UDP slices over itself ("jumbo_udp").
    jh = bytes([17, 0, 0xC2, 4]) + struct.pack(">I", 99999)
    c.append(("ip6_jumbo_udp_70000", eth(ip6(jh + udp(blob(70000, 9), length=0), 0, length=0x1234), 0x86DD), "jumbo_udp"))
    # 8 Pad1 grow the HopByHop by 8 bytes: "Cannot fit payload into IPv6 header" at Length 65535
    grow = hbh(59, bytes(8) + bytes([1, 4, 0, 0, 0, 0]))
    c.append(("ip6_hbh_grow_fit", eth(ip6(grow + blob(65535, 8), 0, length=65535), 0x86DD), None))
    c.append(("ip6_hbh_grow_ok", eth(ip6(grow + blob(100, 8), 0, length=100), 0x86DD), None))
    c.append(("sum_wraps_ff", eth(ip4(tcp(b"\xff" * 262144), 6, length=0), 0x0800), "wide"))
    for n in (65535, 70000):
        c.append(("ip4_wide_tcp_%d" % n, eth(ip4(tcp(blob(n, 3)), 6, length=0), 0x0800), "wide"))
        c.append(("ip6_wide_udp_%d" % n, eth(ip6(udp(blob(n, 4), length=0), 17, length=65535), 0x86DD), "wide"))
    # IPv4 option lists: IHL 5..15
    for ihl in range(5, 16):
        n = (ihl - 5) * 4
        c.append(("ip4_nop_ihl%d" % ihl, tcp4(9, ihl, ip_opts=b"\x01" * n), None))
        if n:
            c.append(("ip4_eol_pad_ihl%d" % ihl, tcp4(10, ihl, ip_opts=b"\x01\x00" + b"\xA5" * (n - 2)), None))
        if n >= 4:
            c.append(("ip4_tlv_ihl%d" % ihl, tcp4(11, ihl, ip_opts=bytes([0x94, n - 1]) + blob(n - 3, ihl) + b"\x00"), None))
    c.append(("ip4_nop_nop_eol_pad5", tcp4(5, 2, ip_opts=b"\x01\x01\x00" + b"\x77" * 5), None))
    # TCP option lists: DataOffset 5..15
    mss, ts = bytes([2, 4, 5, 0xB4]), bytes([8, 10]) + bytes(range(1, 9))
    for doff in range(5, 16):
        n = (doff - 5) * 4
        c.append(("tcp_nop_doff%d" % doff, tcp4(7, doff, opts=b"\x01" * n), None))
        if n:
            c.append(("tcp_eol_pad_doff%d" % doff, tcp4(8, doff, opts=b"\x00" + b"\x5A" * (n - 1)), None))
            c.append(("tcp_nop_eol_pad_doff%d" % doff, tcp4(8, doff, opts=b"\x01\x00" + b"\xC3" * (n - 2)), None))
        if n >= 16:
            c.append(("tcp_mss_ts_doff%d" % doff, tcp4(6, doff, opts=mss + ts + b"\x01" * (n - 14)), None))
        if n >= 12:  # MP_CAPABLE of 12 bytes re-serializes as two: the header shrinks
            mp = bytes([30, 12, 0x00, 0x81]) + bytes(range(8))
            c.append(("tcp_mptcp_doff%d" % doff, tcp4(13, doff, opts=mp + b"\x01" * (n - 12)), None))
            if n >= 16:
                c.append(("tcp_mptcp_eol_doff%d" % doff, tcp4(13, doff, opts=mp + b"\x00" + b"\x99" * (n - 13)), None))
    c.append(("tcp_3nop_eol_pad4", tcp4(8, 3, opts=b"\x01\x01\x01\x00" + b"\x5A" * 4), None))
    # HopByHop: Pad1, PadN, 24 and 32 bytes
    u = udp(blob(21, 2), pseudo=IP6_A + IP6_B)
    for name, h in (("padn", hbh(17, bytes([1, 4, 0, 0, 0, 0]))),
                    ("pad1", hbh(17, bytes([0, 0, 1, 2, 0, 0]))),
                    ("pad1x6", hbh(17, bytes(6))),
                    ("tlv", hbh(17, bytes([0x1E, 4, 9, 8, 7, 6]))),
                    ("24", hbh(17, bytes([1, 4, 0, 0, 0, 0]) + bytes([0x1E, 6]) + bytes(range(6)) + bytes([1, 6]) + bytes(6))),
                    ("24_pad1", hbh(17, bytes(8) + bytes([1, 4, 0, 0, 0, 0]) + bytes([1, 6]) + bytes(6))),
                    ("32", hbh(17, bytes([1, 28]) + bytes(28)))):
        c.append(("hbh_%s" % name, eth(ip6(h + u, 0), 0x86DD), None))
    # stacked layers and gaps
    c.append(("qinq", eth(vlan(vlan(ip4(tcp(blob(33, 9), pseudo=P4), 6), 0x0800, 0x2005), 0x8100, 0xE00A), 0x88A8), None))
    c.append(("vlan", eth(vlan(ip4(udp(blob(17, 9), pseudo=P4), 17), 0x0800), 0x8100), None))
    c.append(("vlan_pop", eth(vlan(ip4(udp(blob(17, 9), pseudo=P4), 17), 0x0800), 0x8100), _vlan_pop))
    inner = ip4(tcp(blob(40, 10), pseudo=P4), 6)
    c.append(("ip4_in_ip4", eth(ip4(inner, 4, src=bytes([1, 1, 1, 1]), dst=bytes([2, 2, 2, 2])), 0x0800), None))
    c.append(("ip4_in_ip4_opts", eth(ip4(inner, 4, opts=b"\x01\x01\x01\x00"), 0x0800), None))
    c.append(("6in4", eth(ip4(ip6(udp(blob(31, 11), pseudo=IP6_A + IP6_B), 17), 41), 0x0800), None))
    c.append(("4in6", eth(ip6(ip4(udp(blob(31, 12), pseudo=P4), 17), 4), 0x86DD), None))
    dest = bytes([17, 0, 1, 4, 0, 0, 0, 0])
    c.append(("ip6_dest_udp", eth(ip6(dest + udp(blob(27, 13), pseudo=IP6_A + IP6_B), 60), 0x86DD), None))
    frag = bytes([6, 0, 0, 0, 0, 0, 0, 7])  # an IPv6 fragment header, offset 0: the skipper walks it
    c.append(("ip6_frag_tcp", eth(ip6(frag + tcp(blob(19, 14), pseudo=IP6_A + IP6_B), 44), 0x86DD), None))
    # an odd-length gap in front of the transport header: a 5-byte stretch the layout skips. The IPv4 slice
    # is handed over with IHL 5 while the layout's TCP starts 5 bytes later: built by moving the layout.
    c.append(("odd_gap", eth(ip4(b"\xAB\xCD\xEF\x01\x23" + tcp(blob(23, 15), pseudo=P4), 6), 0x0800), "odd_gap"))
    # edits
    c.append(("dnat4", tcp4(100, 20), _set(ip4_dst=[172, 16, 0, 99])))
    c.append(("snat4_udp_port", udp4(51, 21), _set(ip4_src=[8, 8, 4, 4], udp_src_port=1024, udp_dst_port=65535)))
    c.append(("nat6", udp6(45, 22), _set(ip6_dst=list(bytes.fromhex("fd000000000000000000000000000042")))))
    c.append(("tcp6_ports", eth(ip6(tcp(blob(37, 23), pseudo=IP6_A + IP6_B), 6), 0x86DD),
              _set(tcp_src_port=80, tcp_dst_port=8080, ip6_hop_limit=1, ip6_flow_label=0xFFFFF, ip6_traffic_class=0xFF)))
    c.append(("ttl_dec", tcp4(64, 24), _set(ip4_ttl=63)))
    c.append(("clear_tcp", tcp4(30, 25), _clear(TCP)))
    c.append(("clear_udp6", udp6(30, 26), _clear(UDP)))
    c.append(("clear_ip4_keep_tcp", tcp4(30, 27), _clear(IP4)))  # ComputeChecksums: no network layer
    c.append(("clear_ip6_in_6in4", eth(ip4(ip6(udp(blob(31, 11)), 17), 41), 0x0800), _clear(IP6)))  # pseudo-header: IPv4
    c.append(("clear_eth", tcp4(12, 28), _clear(ETH)))
    c.append(("set_d1q_no_slice", tcp4(12, 29), _setbit(D1Q)))
    c.append(("set_udp_no_slice", tcp4(12, 30), _setbit(UDP)))
    c.append(("8023", eth(b"\xAA\xAA\x03" + blob(40, 31), 43), None))
    c.append(("8023_trailer", eth(b"\xAA\xAA\x03" + blob(40, 31) + b"\x11" * 7, 43), None))
    c.append(("8023_long", eth(blob(0x5DC, 32), 0x5DC), None))
    c.append(("8023_type_conflict", eth(blob(50, 33), 50), _set(eth_type=0x0800)))
    c.append(("eth_length_on_typed", tcp4(12, 34), _set(eth_length=77)))
    c.append(("eth_length_too_long", eth(blob(50, 33), 50), _set(eth_length=0x0601)))
    c.append(("no_layers", b"\x01\x02\x03", None))
    c.append(("empty", b"", None))
    return c


def aligned_tails():
    """[(name, packet, source alignment)] with the fillers that set the output offsets (see the module's text)"""
    out = []
    at = 0  # the output offset so far, mod 16
    for ln in list(range(0, 71)) + list(range(1440, 1481)):
        for d in range(16):
            fill = (d - at) % 16
            while fill:  # undecodable: serializes to its own bytes
                k = min(fill, 13)
                out.append(("fill", bytes([0xF0 + k]) * k, 0))
                fill -= k
            pkt = udp4(ln, ln) if ln & 1 else tcp4(ln, ln, opts=b"\x01\x01\x01\x00" if ln % 3 == 0 else b"")
            out.append(("tail_%d_d%d" % (ln, d), pkt, (d + ln) % 16))
            at = (d + max(len(pkt), 60)) % 16
    return out


def pack_at(packets, aligns):
    offs, off = [], 0
    for p, a in zip(packets, aligns):
        off += (a - off) % 16
        offs.append(off)
        off += len(p)
    data = np.zeros(off + 64, np.uint8)
    for o, p in zip(offs, packets):
        data[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return data, np.array(offs, np.uint64), np.array([len(p) for p in packets], np.uint32)


def decode(data, offsets, caplens, move=None):
    """the oracle's layouts (move(layouts) may edit them) and the fields records extracted from them"""
    r = O.OracleParser(17, DECODERS).decode(data, offsets, caplens)
    layouts = r["layouts"].copy()
    if move is not None:
        move(layouts)
    f = O.extract_fields(data, offsets, layouts).view(_lib.FIELDS_DTYPE).reshape(-1).copy()
    return layouts, f


_built = {}


def build(which="cases"):
    """dict(data, offsets, caplens, layouts, fields, names) of cases() or aligned_tails(); built once, shared"""
    if which in _built:
        return _built[which]
    if which == "cases":
        cs = cases()
        names, pkts, edits = [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]
        aligns = [(3 * i + 1) % 16 for i in range(len(pkts))]
    else:
        cs = aligned_tails()
        names, pkts, aligns = [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]
        edits = [None] * len(pkts)
    data, offsets, caplens = pack_at(pkts, aligns)
    def move(layouts):
        for i, e in enumerate(edits):
            if e == "odd_gap":  # the TCP header 5 bytes into the IPv4 payload: a slice the caller moved
                layouts[i]["start"][TCP] = 14 + 20 + 5
                layouts[i]["end"][TCP] = caplens[i]
                layouts[i]["start"][PAY] = _lib.LAYOUT_ABSENT
            if e == "jumbo_udp":
                layouts[i]["start"][IP6], layouts[i]["end"][IP6] = 14, caplens[i]
                layouts[i]["start"][UDP], layouts[i]["end"][UDP] = 14 + 48, caplens[i]
                layouts[i]["start"][PAY] = _lib.LAYOUT_ABSENT
            if e == "wide":  # the transport slice runs to the end of the packet
                for k in (TCP, UDP):
                    if layouts[i]["start"][k] != _lib.LAYOUT_ABSENT:
                        layouts[i]["end"][k] = caplens[i]

    layouts, fields = decode(data, offsets, caplens, move)
    for i, e in enumerate(edits):
        if e == "jumbo_udp":  # a Length FixLengths has to replace by 0
            fields[i]["udp_length"] = 999
        if e is not None and not isinstance(e, str):
            e(fields[i])
    _built[which] = dict(data=data, offsets=offsets, caplens=caplens, layouts=layouts, fields=fields, names=names)
    return _built[which]
