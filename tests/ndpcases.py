"""Hand-derived NDP / MLD packets, one per error site, quirk and layer of
include/gpk_ndp.h, and the seeded corpus of the NDP tests.

Every case is (name, packet bytes). The expected values come from
ndp_model.py; EXPECT also carries the outcome by hand (class, layer type, error
code and arguments, status bits, entries, a few fields), derived from the
reference's source, so the model is checked too.

The parser routes ten private EtherTypes straight to the ten message layers
(gpk_parser_set_ethertype): way 2 of the candidate rule, and the only way to an
MLDv1 query with a payload. controlcases' edits (ICMPv6 without a network
layer) are kept.
"""
import random
import struct

import controlcases as CC
from controlcases import MAC, eth, hbh, icmp6, ip4, ip6, udp, vxlan, over_udp  # noqa: F401

(LT_RS, LT_RA, LT_NS, LT_NA, LT_REDIRECT) = range(124, 129)
LT_MLD1_REPORT, LT_MLD1_DONE, LT_MLD1_QUERY, LT_MLD2_REPORT, LT_MLD2_QUERY = range(135, 140)
LAYER_TYPES = (LT_RS, LT_RA, LT_NS, LT_NA, LT_REDIRECT, LT_MLD1_QUERY, LT_MLD1_REPORT, LT_MLD1_DONE, LT_MLD2_QUERY,
               LT_MLD2_REPORT)
ET_OF = {lt: 0x9900 + lt for lt in LAYER_TYPES}   # way 2: EtherType -> the message layer itself
ICMP_TYPE = {LT_RS: 133, LT_RA: 134, LT_NS: 135, LT_NA: 136, LT_REDIRECT: 137, LT_MLD1_QUERY: 130, LT_MLD1_REPORT: 131,
             LT_MLD1_DONE: 132, LT_MLD2_QUERY: 130, LT_MLD2_REPORT: 143}
EDITS = dict(list(CC.EDITS.items()) + [(et, lt) for lt, et in ET_OF.items()])
PARSER = dict(CC.PARSER, ethertype=EDITS)
PARSER_IGNORE = dict(PARSER, ignore_unsupported=True)
PARSER_NOPAYLOAD = dict(PARSER, decoders=[d for d in PARSER["decoders"] if d != "PAYLOAD"])

TARGET = bytes.fromhex("fe80000000000000020c29fffe0e4c67")
DEST = bytes.fromhex("20010db8000000010000000000000099")
GROUP = bytes.fromhex("ff020000000000000000000000010003")
GROUP2 = bytes.fromhex("ff0200000000000000000001ffcce546")
LLADDR = bytes.fromhex("000c290e4c67")


def opt(typ, data):
    """One option; len(data) + 2 is a multiple of 8."""
    assert (len(data) + 2) % 8 == 0
    return bytes([typ, (len(data) + 2) // 8]) + data


def opt_lladdr(typ=1, mac=LLADDR):
    return opt(typ, mac)


def opt_mtu(mtu=1500):
    return opt(5, bytes(2) + struct.pack(">I", mtu))


def opt_prefix(prefix=bytes.fromhex("20010db8000000010000000000000000"), plen=64, flags=0xc0, valid=2592000,
               preferred=604800):
    return opt(3, struct.pack(">BBIII", plen, flags, valid, preferred, 0) + prefix)


def opt_rdnss(servers=(bytes.fromhex("20010db8000000000000000000000053"),), lifetime=600):
    return opt(25, bytes(2) + struct.pack(">I", lifetime) + b"".join(servers))


def rs(options=b""):
    return bytes(4) + options


def ra(options=b"", hop=64, flags=0x40, lifetime=1800, reachable=30000, retrans=1000):
    return struct.pack(">BBHII", hop, flags, lifetime, reachable, retrans) + options


def ns(options=b"", target=TARGET):
    return bytes(4) + target + options


def na(options=b"", target=TARGET, flags=0x60):
    return bytes([flags, 0, 0, 0]) + target + options


def redirect(options=b"", target=TARGET, dest=DEST):
    return bytes(4) + target + dest + options


def mld1(group=GROUP, delay=10000):
    return struct.pack(">HH", delay, 0) + group


def mld2_query(sources=(), group=GROUP, code=10000, s_qrv=0x0a, qqic=60, count=None):
    return struct.pack(">HH", code, 0) + group + struct.pack(">BBH", s_qrv, qqic,
                                                            len(sources) if count is None else count) + b"".join(sources)


def record(group=GROUP, sources=(), aux=b"", typ=2, n=None, aux_len=None):
    return struct.pack(">BBH", typ, len(aux) // 4 if aux_len is None else aux_len,
                       len(sources) if n is None else n) + group + b"".join(sources) + aux


def mld2_report(records=(), count=None):
    return struct.pack(">HH", 0, len(records) if count is None else count) + b"".join(records)


def behind(lt, body, **kw):
    """Way 1: Ethernet, IPv6, ICMPv6 of the layer's type, the message."""
    return eth(ip6(icmp6(body, ICMP_TYPE[lt], **kw), 58), 0x86dd)


def front(lt, body):
    """Way 2: the message straight behind Ethernet, through the table edit."""
    return eth(body, ET_OF[lt])


SRC_A, SRC_B = bytes.fromhex("20010db8" + "00" * 11 + "0a"), bytes.fromhex("20010db8" + "00" * 11 + "0b")
HDR = 14 + 40 + 4   # the message's packet offset behind Ethernet, IPv6 and the ICMPv6 header


def quirk_cases():
    c = []
    E = {}

    def add(name, pkt, **expect):
        c.append((name, pkt))
        if expect:
            E[name] = expect
    three = opt_lladdr() + opt_mtu() + opt_prefix()
    # ---- Router Solicitation (icmp6msg.go:190-202) and Advertisement (:237-255)
    for k in (1, 2, 3):
        add("rs_%d_bytes" % k, behind(LT_RS, bytes(k)), cls=1, lt=LT_RS, err=140, status=1, hdr=HDR)
    add("rs_4_bytes_no_options", behind(LT_RS, rs()), cls=0, lt=LT_RS, nentries=0, contents=0, len=4)
    add("rs_12_bytes_one_option", behind(LT_RS, rs(opt_lladdr())), cls=0, lt=LT_RS, nentries=1, contents=0, len=12,
        entries=[(1, HDR + 6, 6)])
    for k in (1, 2, 3, 4):
        add("ra_%d_bytes" % k, behind(LT_RA, ra()[:k]), cls=1, lt=LT_RA, err=141, status=1)
    add("ra_11_bytes", behind(LT_RA, ra()[:11]), cls=1, err=141, status=1)
    add("ra_12_bytes_no_options", behind(LT_RA, ra()), cls=0, lt=LT_RA, nentries=0, contents=12, len=12, flags=0x40,
        v=[30000, 1000, 1800, 64])
    add("ra_three_options", behind(LT_RA, ra(three)), cls=0, lt=LT_RA, nentries=3, contents=12 + 48,
        entries=[(1, HDR + 14, 6), (5, HDR + 22, 6), (3, HDR + 30, 30)])
    add("ra_four_options_rdnss", behind(LT_RA, ra(three + opt_rdnss(), flags=0x80)), cls=0, nentries=4, flags=0x80)
    # ---- Neighbor Solicitation (:306-319) and Advertisement (:355-369)
    add("ns_19_bytes", behind(LT_NS, ns()[:19]), cls=1, lt=LT_NS, err=142, status=1)
    add("ns_20_bytes", behind(LT_NS, ns()), cls=0, lt=LT_NS, nentries=0, contents=20, v=[HDR + 4, 0, 0, 0])
    add("ns_one_option", behind(LT_NS, ns(opt_lladdr())), cls=0, nentries=1, entries=[(1, HDR + 22, 6)])
    add("na_19_bytes", behind(LT_NA, na()[:19]), cls=1, lt=LT_NA, err=143, status=1)
    add("na_20_bytes", behind(LT_NA, na()), cls=0, lt=LT_NA, nentries=0, contents=20, flags=0x60, v=[HDR + 4, 0, 0, 0])
    add("na_target_option", behind(LT_NA, na(opt_lladdr(2), flags=0xe0)), cls=0, nentries=1, flags=0xe0,
        entries=[(2, HDR + 22, 6)])
    # ---- Redirect (:422-436)
    add("redirect_35_bytes", behind(LT_REDIRECT, redirect()[:35]), cls=1, lt=LT_REDIRECT, err=144, status=1)
    add("redirect_36_bytes", behind(LT_REDIRECT, redirect()), cls=0, lt=LT_REDIRECT, nentries=0, contents=36,
        v=[HDR + 4, HDR + 20, 0, 0])
    add("redirect_header_option", behind(LT_REDIRECT, redirect(opt_lladdr(2) + opt(4, bytes(6) + bytes(range(40))))),
        cls=0, nentries=2, entries=[(2, HDR + 38, 6), (4, HDR + 46, 46)])
    # ---- the options' own error sites (:514-546)
    add("option_length_0", behind(LT_NS, ns(opt_lladdr() + b"\x01\x00" + bytes(6))), cls=1, lt=LT_NS, err=146, status=1,
        nentries=0)
    add("option_overruns_by_one", behind(LT_NS, ns(opt_lladdr() + opt_prefix()[:31])), cls=1, err=147, a0=31, a1=32,
        status=1)
    add("option_one_byte_left", behind(LT_RA, ra(opt_mtu() + b"\x01")), cls=1, lt=LT_RA, err=145, status=1)
    add("option_max_length", behind(LT_RS, rs(bytes([9, 255]) + bytes(2038))), cls=0, nentries=1,
        entries=[(9, HDR + 6, 2038)])
    add("option_255_units_short", behind(LT_RS, rs(bytes([9, 255]) + bytes(2037))), cls=1, err=147, a0=2039, a1=2040)
    # ---- type 130: the payload's length chooses the layer (icmp6.go:249-254)
    add("mld_query_20_is_v1", behind(LT_MLD1_QUERY, mld1()), cls=0, lt=LT_MLD1_QUERY, contents=0, payload_len=0,
        v=[HDR + 4, 0, 10000, 0], nentries=0)
    for k in (21, 22, 23):
        add("mld_query_%d_is_v2_short" % k, behind(LT_MLD2_QUERY, mld2_query()[:k]), cls=1, lt=LT_MLD2_QUERY, err=149,
            status=1)
    add("mld_query_24_is_v2", behind(LT_MLD2_QUERY, mld2_query()), cls=0, lt=LT_MLD2_QUERY, count=0, s_qrv=0x0a, qqic=60,
        v=[HDR + 4, 0, 10000, 0], nentries=0, contents=0)
    add("mld2_query_two_sources", behind(LT_MLD2_QUERY, mld2_query((SRC_A, SRC_B), s_qrv=0xf7)), cls=0, count=2,
        s_qrv=7, len=56)
    add("mld2_query_65535_sources_over_40_bytes", behind(LT_MLD2_QUERY, mld2_query((SRC_A,), count=65535)), cls=1,
        err=150, a0=56, status=1)
    add("mld2_query_source_cut", behind(LT_MLD2_QUERY, mld2_query((SRC_A, SRC_B))[:55]), cls=1, err=150, a0=56)
    add("mld2_query_trailing_bytes", behind(LT_MLD2_QUERY, mld2_query((SRC_A,)) + b"tail"), cls=0, count=1, len=44)
    # ---- MLDv1 Report and Done (mldv1.go:32-43): the same text
    add("mld1_report", behind(LT_MLD1_REPORT, mld1()), cls=0, lt=LT_MLD1_REPORT, v=[HDR + 4, 0, 10000, 0])
    add("mld1_report_19", behind(LT_MLD1_REPORT, mld1()[:19]), cls=1, lt=LT_MLD1_REPORT, err=148, status=1)
    add("mld1_report_trailing", behind(LT_MLD1_REPORT, mld1() + bytes(5)), cls=0, payload_len=0, len=25)
    add("mld1_done", behind(LT_MLD1_DONE, mld1(delay=0)), cls=0, lt=LT_MLD1_DONE, v=[HDR + 4, 0, 0, 0])
    add("mld1_done_3", behind(LT_MLD1_DONE, mld1()[:3]), cls=1, lt=LT_MLD1_DONE, err=148, status=1)
    # ---- MLDv2 Report (mldv2.go:309-333, 473-509)
    add("mld2_report_3_bytes", behind(LT_MLD2_REPORT, mld2_report()[:3]), cls=1, lt=LT_MLD2_REPORT, err=151, status=1)
    add("mld2_report_0_records", behind(LT_MLD2_REPORT, mld2_report()), cls=0, lt=LT_MLD2_REPORT, count=0, nentries=0,
        contents=0)
    two = (record(GROUP, (SRC_A, SRC_B), b"auxd", typ=1), record(GROUP2, typ=4))
    add("mld2_report_2_records", behind(LT_MLD2_REPORT, mld2_report(two)), cls=0, count=2, nentries=2,
        entries=[(1, HDR + 8, HDR + 24, HDR + 56, 1, 2), (4, HDR + 64, HDR + 80, HDR + 80, 0, 0)])  # the second at 60
    add("mld2_report_record_cut_at_19", behind(LT_MLD2_REPORT, mld2_report((record(),))[:4 + 19]), cls=1, err=152,
        status=1)
    add("mld2_report_count_overstates", behind(LT_MLD2_REPORT, mld2_report((record(),), count=2)), cls=1, err=152,
        status=1, nentries=0)
    add("mld2_report_second_source_cut", behind(LT_MLD2_REPORT, mld2_report((record(GROUP, (SRC_A, SRC_B)),))[:4 + 51]),
        cls=1, err=153, a0=52, status=1)
    add("mld2_report_aux_overruns", behind(LT_MLD2_REPORT, mld2_report((record(GROUP, (SRC_A,), b"aux!", aux_len=2),))),
        cls=1, err=154, a0=36, status=0)
    add("mld2_report_second_record_aux_overruns",
        behind(LT_MLD2_REPORT, mld2_report((record(), record(GROUP2, aux_len=255)))), cls=1, err=154, a0=20, status=0)
    # ---- the ICMPv6 header in front
    add("behind_hopbyhop", eth(ip6(hbh(58) + icmp6(ns(opt_lladdr()), 135), 0), 0x86dd), cls=0, lt=LT_NS, hdr=HDR + 8,
        nentries=1)
    add("icmp6_header_only", eth(ip6(icmp6(b"", 135), 58), 0x86dd))              # empty payload: the loop ends
    add("icmp6_3_bytes", eth(ip6(icmp6(b"", 135)[:3], 58), 0x86dd))              # the ICMPv6 itself fails
    add("icmp6_echo", eth(ip6(CC.echo6(), 58), 0x86dd))                          # next type is not one of the ten
    add("icmp6_no_network_layer", eth(icmp6(na(), 136), CC.ET_ICMP6), cls=0, lt=LT_NA, hdr=14 + 4)
    add("icmp6_bad_checksum_still_decodes", behind(LT_NS, ns(), good=False), cls=0, lt=LT_NS)
    add("inside_ipv4", eth(ip4(icmp6(rs(), 133), 58)), cls=0, lt=LT_RS, hdr=14 + 20 + 4)
    # ---- way 2: a table edit leads to the layer itself
    for lt, body in ((LT_RS, rs(opt_lladdr())), (LT_RA, ra(three)), (LT_NS, ns()), (LT_NA, na(opt_lladdr(2))),
                     (LT_REDIRECT, redirect()), (LT_MLD1_REPORT, mld1()), (LT_MLD1_DONE, mld1()),
                     (LT_MLD2_QUERY, mld2_query((SRC_A,))), (LT_MLD2_REPORT, mld2_report(two))):
        add("front_%d" % lt, front(lt, body), cls=0, lt=lt, hdr=14, len=len(body))
    add("front_mld1_query_20", front(LT_MLD1_QUERY, mld1()), cls=0, lt=LT_MLD1_QUERY, hdr=14, payload_len=0)
    add("front_mld1_query_payload", front(LT_MLD1_QUERY, mld1() + b"payload!"), cls=0, lt=LT_MLD1_QUERY, hdr=14,
        payload_off=34, payload_len=8, len=28, contents=0)
    add("front_mld2_query_20_bytes", front(LT_MLD2_QUERY, mld1()), cls=1, lt=LT_MLD2_QUERY, err=149, status=1)
    add("front_ns_19", front(LT_NS, ns()[:19]), cls=1, lt=LT_NS, err=142, status=1, hdr=14)
    # ---- not candidates
    add("plain_udp", eth(ip4(udp(bytes(12), 50004, 53), 17)))
    add("arp", eth(CC.arp(), 0x0806))
    add("icmp6_unknown_type", eth(ip6(icmp6(bytes(20), 200), 58), 0x86dd))
    return c, E


def layers17():
    """Ethernet, 14 Dot1Q tags, IPv6: 16 layers, the ICMPv6 would be the 17th; and one tag more (UNKNOWN)."""
    tags = lambda n: MAC + b"".join(b"\x81\x00" + b"\x00\x05" for _ in range(n)) + b"\x86\xdd"  # noqa: E731
    return tags(14) + ip6(icmp6(ns(opt_lladdr()), 135), 58), tags(15) + ip6(icmp6(ns(opt_lladdr()), 135), 58)


def bodies(rnd):
    """One well-formed message of a random layer: (layer type, body)."""
    def options():
        pool = [opt_lladdr, lambda: opt_lladdr(2), opt_mtu, opt_prefix, opt_rdnss,
                lambda: opt(rnd.randrange(256), bytes(rnd.randrange(256) for _ in range(6 + 8 * rnd.randrange(3))))]
        return b"".join(rnd.choice(pool)() for _ in range(rnd.choice([0, 1, 1, 2, 3, 4])))

    def sources():
        return tuple(bytes(rnd.randrange(256) for _ in range(16)) for _ in range(rnd.choice([0, 0, 1, 2, 3])))

    lt = rnd.choice(LAYER_TYPES)
    if lt == LT_RS:
        return lt, rs(options())
    if lt == LT_RA:
        return lt, ra(options(), rnd.randrange(256), rnd.randrange(256), rnd.randrange(65536))
    if lt == LT_NS:
        return lt, ns(options())
    if lt == LT_NA:
        return lt, na(options(), flags=rnd.randrange(256))
    if lt == LT_REDIRECT:
        return lt, redirect(options())
    if lt in (LT_MLD1_QUERY, LT_MLD1_REPORT, LT_MLD1_DONE):
        return lt, mld1(delay=rnd.randrange(65536))
    if lt == LT_MLD2_QUERY:
        return lt, mld2_query(sources(), code=rnd.randrange(65536), s_qrv=rnd.randrange(256), qqic=rnd.randrange(256))
    recs = tuple(record(rnd.choice([GROUP, GROUP2]), sources(), bytes(4 * rnd.choice([0, 0, 0, 1, 2])),
                        typ=rnd.randrange(1, 8)) for _ in range(rnd.choice([0, 1, 2, 3, 4])))
    return lt, mld2_report(recs)


def corpus(seed, n, vectors=()):
    """The cases and the vectors as they are, with bytes changed or cut short,
    and generated messages of every layer, whole, with a count or length byte
    changed, or cut near the end. `vectors`: packets (bytes) to mix in."""
    rnd = random.Random(seed)
    base = [p for _, p in quirk_cases()[0]] + list(vectors)
    out = []
    while len(out) < n:
        r = rnd.random()
        if r < 0.25:
            pkt = bytearray(rnd.choice(base))
            how = rnd.random()
            if how < 0.3 and len(pkt) > 58:
                for _ in range(rnd.randrange(1, 3)):
                    pkt[rnd.randrange(54, len(pkt))] = rnd.randrange(256)
            elif how < 0.6:
                pkt = pkt[:rnd.randrange(max(1, len(pkt) - 24), len(pkt) + 1)]
            out.append(bytes(pkt))
            continue
        lt, body = bodies(rnd)
        body = bytearray(body)
        how = rnd.random()
        if how < 0.25 and body:      # a byte of the message changed: counts, lengths and types included
            body[rnd.randrange(len(body))] = rnd.choice([0, 1, 2, 3, 255, rnd.randrange(256)])
        elif how < 0.45:             # cut near its end or near its fixed part
            body = body[:rnd.choice([rnd.randrange(0, len(body) + 1), max(0, len(body) - rnd.randrange(1, 18)),
                                     rnd.randrange(0, 40)])]
        elif how < 0.5:              # bytes added behind it
            body += bytes(rnd.randrange(1, 9))
        body = bytes(body)
        w = rnd.random()
        if w < 0.25:
            out.append(front(lt, body))
        elif w < 0.35:
            out.append(eth(ip6(hbh(58) + icmp6(body, ICMP_TYPE[lt]), 0), 0x86dd))
        elif w < 0.4:
            out.append(eth(icmp6(body, ICMP_TYPE[lt]), CC.ET_ICMP6))
        else:
            out.append(behind(lt, body))
    return out


CORPUS_SEED = 20261021
CORPUS_N = 2048
