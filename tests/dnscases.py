"""Hand-built DNS messages: one per error code of include/gpk_dns.h, one per
quirk of its rules, one per record type, and the seeded
mutation corpus of the DNS tests.

Every case is (name, packet bytes). The expected arrays come from
dns_model.py; EXPECT also carries, by hand from the reference's source, each
case's error code and arguments (0: it decodes), and for some the entry names,
the RDATA names and the response code, so the model is checked too.

The parser sends TCP port 8080 to LayerTypeDNS (gpk_parser_set_tcp_port): the
table-edited port.
"""
import random
import struct

from tunnelcases import MAC, eth, ip4, ip6, tcp, udp, vxlan, over_udp, VX  # noqa: F401

PARSER = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"],
              tcp_port={8080: 107})
PARSER_IGNORE = dict(PARSER, ignore_unsupported=True)
PARSER_NOPAYLOAD = dict(PARSER, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP"])
(A, NS, CNAME, SOA, NULL, PTR, HINFO, MX, TXT, AAAA, SRV, NAPTR, OPT, RRSIG, DNSKEY, SVCB, HTTPS, URI) = (
    1, 2, 5, 6, 10, 12, 13, 15, 16, 28, 33, 35, 41, 46, 48, 64, 65, 256)


def name(*labels, ptr=None):
    """Wire labels, ended by a pointer to message offset `ptr` or by the root."""
    out = b"".join(bytes([len(x)]) + x for x in labels)
    return out + (struct.pack(">H", 0xc000 | ptr) if ptr is not None else b"\x00")


def hdr(qd=0, an=0, ns=0, ar=0, ident=0x1234, flags=0x8180):
    return struct.pack(">HHHHHH", ident, flags, qd, an, ns, ar)


def q(nm, typ=A, cls=1):
    return nm + struct.pack(">HH", typ, cls)


def rr(nm, typ, rdata=b"", cls=1, ttl=300, dl=None):
    return nm + struct.pack(">HHIH", typ, cls, ttl, len(rdata) if dl is None else dl) + rdata


def over(msg, sport=50004, dport=53):
    return eth(ip4(udp(msg, sport, dport), 17))


def over_tcp(msg, dport=53):
    return eth(ip4(tcp(struct.pack(">H", len(msg)) + msg, dport=dport), 6))


EX = name(b"example", b"com")     # at offset 12 of a message that starts with q(EX): "example.com"
QEX = q(EX)                       # 17 bytes: the answers start at 29
P = name(ptr=12)                  # a pointer to it
OPT0 = b"\x00"                    # the root owner of an OPT record


def answer(typ, rdata, **kw):
    """A response to q(EX) with one answer of `typ`; its RDATA starts at 29 + 2 + 10 = 41."""
    return hdr(1, 1) + QEX + rr(P, typ, rdata, **kw)


def loop_message():
    """The deepest walk a 1500-byte message allows: a level of 126 one-byte
    labels that ends in a pointer to its own start. 255 levels of 126 labels,
    then level 256 fails."""
    return hdr(1, 0) + b"\x01a" * 126 + name(ptr=12) + struct.pack(">HH", A, 1)


def chain_message(levels):
    """A question name whose pointer chain ends with label "x" at `levels`: level 1 is
    the pointer in the question, the chain lies behind the question, where nothing else reads."""
    t = 12 + 2 + 4
    chain = b"".join(name(ptr=t + 2 * (k + 1)) for k in range(levels - 2)) + name(b"x")
    return hdr(1, 0) + q(name(ptr=t)) + chain


def quirk_cases():
    c = []
    E = {}

    def add(nm, pkt, **expect):
        c.append((nm, pkt))
        E[nm] = expect
    # ---- one per record type (decodeRData, dns.go:1350-1529)
    add("query_a", over(hdr(1, flags=0x0100) + QEX), err=0, names=[b"example.com"])
    add("resp_a", over(answer(A, bytes([192, 0, 2, 1]))), err=0, names=[b"example.com", b"example.com"])
    add("resp_aaaa", over(answer(AAAA, bytes(range(16)))), err=0)
    add("resp_ns", over(answer(NS, name(b"ns1", ptr=12))), err=0, rnames=[b"", b"ns1.example.com"])
    add("resp_cname", over(answer(CNAME, name(b"www", b"example", b"org"))), err=0, rnames=[b"", b"www.example.org"])
    add("resp_ptr", over(answer(PTR, name(b"host", ptr=20))), err=0, rnames=[b"", b"host.com"])
    add("resp_txt", over(answer(TXT, b"\x03abc\x00\x05hello")), err=0, counts=[0, 3])
    add("resp_hinfo", over(answer(HINFO, b"\x03cpu\x02os")), err=0, counts=[0, 2])
    add("resp_soa", over(answer(SOA, name(b"ns", ptr=12) + name(b"admin", ptr=12) + struct.pack(">IIIII", 1, 2, 3, 4, 5))),
        err=0, rnames=[b"", b"ns.example.com"], rnames2=[b"", b"admin.example.com"])
    add("resp_mx", over(answer(MX, struct.pack(">H", 10) + name(b"mail", ptr=12))), err=0, rnames=[b"", b"mail.example.com"])
    add("resp_srv", over(answer(SRV, struct.pack(">HHH", 1, 2, 5060) + name(b"sip", ptr=12))), err=0,
        rnames=[b"", b"sip.example.com"])
    add("resp_naptr", over(answer(NAPTR, struct.pack(">HH", 100, 10) + b"\x01u\x07E2U+sip\x04!^.!" + name(b"r", ptr=12))),
        err=0, rnames=[b"", b"r.example.com"])
    add("resp_naptr_empty_strings", over(answer(NAPTR, struct.pack(">HH", 1, 2) + b"\x00\x00\x00" + b"\x00")), err=0)
    add("resp_opt", over(hdr(1, 0, 0, 1) + QEX + rr(OPT0, OPT, struct.pack(">HH", 10, 8) + bytes(8) + struct.pack(">HH", 12, 0),
                                                   cls=4096, ttl=0)), err=0, counts=[0, 2])
    add("resp_rrsig", over(answer(RRSIG, struct.pack(">HBBIIIH", A, 8, 2, 300, 1700000000, 1690000000, 4242) +
                                  name(b"example", b"com") + b"signature-bytes")), err=0, rnames=[b"", b"example.com"])
    add("resp_rrsig_root_signer", over(answer(RRSIG, struct.pack(">HBBIIIH", A, 8, 0, 1, 2, 3, 4) + b"\x00" + b"sig")),
        err=0, rnames=[b"", b""])
    add("resp_rrsig_one_byte_signer", over(answer(RRSIG, struct.pack(">HBBIIIH", A, 8, 1, 1, 2, 3, 4) + name(b"a") + b"s")),
        err=0, rnames=[b"", b"a"])  # the buffer is ".a": longer than 1, the dot goes
    add("resp_dnskey", over(answer(DNSKEY, struct.pack(">HBB", 257, 3, 13) + bytes(range(32)))), err=0)
    add("resp_svcb", over(answer(SVCB, struct.pack(">H", 1) + name(b"svc", ptr=12) + struct.pack(">HH", 1, 3) + b"\x02h2" +
                                 struct.pack(">HH", 3, 2) + struct.pack(">H", 443))), err=0, counts=[0, 2],
        rnames=[b"", b"svc.example.com"])
    add("resp_https_alias", over(answer(HTTPS, struct.pack(">H", 0) + name(b"alias", ptr=12))), err=0, counts=[0, 0])
    add("resp_uri", over(answer(URI, struct.pack(">HH", 10, 1) + b"https://example.com/")), err=0)
    add("resp_unknown_type", over(answer(NULL, b"\xc0\xff\xff")), err=0)  # no decodeRData case: bytes only
    add("resp_all_sections", over(hdr(1, 2, 1, 1) + QEX + rr(P, A, bytes(4)) + rr(P, A, bytes([1, 2, 3, 4])) +
                                  rr(P, NS, name(b"ns", ptr=12)) + rr(name(b"ns", ptr=12), A, bytes(4))), err=0,
        names=[b"example.com"] * 4 + [b"ns.example.com"])
    add("resp_over_ipv6", eth(ip6(udp(answer(A, bytes(4)), 53, 40000), 17), 0x86dd), err=0)  # the source port is 53
    # ---- quirks
    # the ID is the length and all shifts by two: QDCount is 0x0100; the first "question" is the root (the header's
    # last zero byte), type 0x0007, class "ex"; the second starts at 17 with 'a' = 0x61, a 0x40 form
    add("tcp_length_prefix", over_tcp(hdr(1, flags=0x0100) + QEX), err=E_OF["Q40"], a0=0x61, a1=17)
    add("tcp_length_prefix_decodes", over_tcp(b"\x00\x00" * 5), err=0, ident=10)  # ID 10, the header is 5 zero words + 2
    add("table_edited_port", eth(ip4(tcp(hdr(1) + QEX, dport=8080), 6)), err=0, names=[b"example.com"])
    add("pointer_to_root", over(hdr(1) + q(name(ptr=16)) + b""), err=0, names=[b""])  # offset 16: the class's zero high byte
    add("chain_ending_at_level_255", over(chain_message(255)), err=0, names=[b"x"])
    add("chain_reaching_level_256", over(chain_message(256)), err=E_OF["MAXREC"])
    add("pointer_loop_255_levels", over(loop_message()), err=E_OF["MAXREC"])
    add("pointer_to_itself", over(hdr(1) + q(name(ptr=12))), err=E_OF["MAXREC"])
    add("offsetp_equals_len", over(hdr(1) + q(name(ptr=18))), err=E_OF["OFFHIGH"])  # 12 + 2 + 4 = 18 = len
    add("offsetp_past_len", over(hdr(1) + q(name(ptr=19))), err=E_OF["PTRHIGH"])
    add("level_of_255_bytes_then_pointer", over(hdr(2) + QEX + q(name(b"a" * 63, b"b" * 63, b"c" * 63, b"d" * 62, ptr=20))),
        err=0, names=[b"example.com", b"a" * 63 + b"." + b"b" * 63 + b"." + b"c" * 63 + b"." + b"d" * 62 + b".com"])
    add("level_of_256_bytes", over(hdr(2) + QEX + q(name(b"a" * 63, b"b" * 63, b"c" * 63, b"d" * 63, ptr=20))),
        err=E_OF["LONG"])
    add("opt_extended_rcode_twice", over(hdr(1, 0, 0, 2, flags=0x8183) + QEX + rr(OPT0, OPT, ttl=0x01000000, cls=1232) +
                                         rr(OPT0, OPT, ttl=0x02000000, cls=1232)), err=0, rcode=0x33)
    add("opt_in_answers_is_no_extension", over(hdr(1, 1, flags=0x8183) + QEX + rr(OPT0, OPT, ttl=0x01000000)), err=0, rcode=3)
    add("data_length_0_typed", over(hdr(1, 3) + QEX + rr(P, MX) + rr(P, SOA) + rr(P, SVCB)), err=0)
    # the CNAME record is message[29:43]: decodeRData sees data[:43], the A record behind it is out of reach
    add("rdata_pointer_past_record_end", over(hdr(1, 2) + QEX + rr(P, CNAME, name(ptr=44)) + rr(P, A, bytes(4))),
        err=E_OF["PTRHIGH"])
    add("rdata_pointer_to_record_end", over(hdr(1, 2) + QEX + rr(P, CNAME, name(ptr=43)) + rr(P, A, bytes(4))),
        err=E_OF["OFFHIGH"])
    add("trailing_bytes_ignored", over(hdr(1) + QEX + b"trailing"), err=0)
    add("counts_zero", over(hdr()), err=0)
    add("label_with_dot_and_backslash", over(hdr(1) + q(name(b"a.b", b"c\\d", b"\x00\xff"))), err=0,
        names=[b"a.b.c\\d.\x00\xff"])
    add("empty_payload", over(b""))                       # not a candidate: the loop ends before the type is looked at
    add("not_dns", over(hdr(1) + QEX, 50004, 5353))       # mDNS is no DNS port unless registered
    add("plain_tcp", eth(ip4(tcp(b"hello"), 6)))
    # ---- one per error code
    add("short_11", over(hdr()[:11]), err=E_OF["SHORT"], status=1)
    add("short_1", over(b"\x00"), err=E_OF["SHORT"], status=1)
    add("name_invalid_index", over(hdr(1) + b"\x05ab"), err=E_OF["INVIDX"])
    add("pointer_cut", over(hdr(1) + b"\x01a\xc0"), err=E_OF["PTRHIGH"])
    add("label_ends_at_len", over(hdr(1) + b"\x03abc"), err=E_OF["RANGE"])
    add("qname_0x40", over(hdr(1) + q(b"\x01a\x41" + EX)), err=E_OF["Q40"], a0=0x41, a1=14)
    add("qname_0x80", over(hdr(1) + q(b"\x85" + EX)), err=E_OF["Q80"], a0=0x85, a1=12)
    add("question_small", over(hdr(1) + QEX[:-1]), err=E_OF["QSMALL"])
    add("question_name_only", over(hdr(1) + EX), err=E_OF["QSMALL"])
    add("record_small", over(answer(A, bytes(4))[:29 + 2 + 9]), err=E_OF["RSMALL"])
    add("record_length_exceeds", over(answer(A, bytes(3), dl=4)), err=E_OF["RLEN"])
    add("an_count_without_records", over(hdr(1, 1) + QEX), err=E_OF["OFFHIGH"])
    add("txt_string_overruns", over(answer(TXT, b"\x03abc\x04xyz")), err=E_OF["CHARSTR"])
    add("soa_small", over(answer(SOA, name(b"ns", ptr=12) + name(b"admin", ptr=12) + bytes(19))), err=E_OF["SOA"])
    add("soa_rname_at_end", over(answer(SOA, name(b"ns", ptr=12))), err=E_OF["OFFHIGH"])
    add("mx_small", over(answer(MX, b"\x00")), err=E_OF["MX"])
    add("mx_no_name", over(answer(MX, b"\x00\x0a")), err=E_OF["OFFHIGH"])
    add("uri_small", over(answer(URI, b"\x00\x0a\x00")), err=E_OF["URI"])
    add("srv_small", over(answer(SRV, bytes(5))), err=E_OF["SRV"])
    add("naptr_small", over(answer(NAPTR, bytes(3))), err=E_OF["NAPTR"])
    add("naptr_flags_missing", over(answer(NAPTR, bytes(4))), err=E_OF["NF_MISS"])
    add("naptr_flags_truncated", over(answer(NAPTR, bytes(4) + b"\x03ab")), err=E_OF["NF_TRUNC"])
    add("naptr_service_missing", over(answer(NAPTR, bytes(4) + b"\x01u")), err=E_OF["NS_MISS"])
    add("naptr_service_truncated", over(answer(NAPTR, bytes(4) + b"\x01u\x02s")), err=E_OF["NS_TRUNC"])
    add("naptr_regexp_missing", over(answer(NAPTR, bytes(4) + b"\x01u\x01s")), err=E_OF["NR_MISS"])
    add("naptr_regexp_truncated", over(answer(NAPTR, bytes(4) + b"\x01u\x01s\x09re")), err=E_OF["NR_TRUNC"])
    add("opt_length_3", over(hdr(1, 0, 0, 1) + QEX + rr(OPT0, OPT, bytes(3))), err=E_OF["OPT_LEN"], a0=3)
    # len(data) is the record's end in the message: 12 + 17 + 11 + 6 = 46; the second option starts at 44
    add("opt_second_option_cut", over(hdr(1, 0, 0, 1) + QEX + rr(OPT0, OPT, struct.pack(">HH", 3, 0) + b"\x00\x03")),
        err=E_OF["OPT_MAL"], a0=46, a1=48)
    add("opt_length_implies_more", over(hdr(1, 0, 0, 1) + QEX + rr(OPT0, OPT, struct.pack(">HH", 3, 10) + b"ab")),
        err=E_OF["OPT_IMPL"], a0=10)
    add("svcb_length_2", over(answer(SVCB, b"\x00\x01")), err=E_OF["SVCB_LEN"], a0=2)
    add("svcb_length_1", over(answer(HTTPS, b"\x00")), err=E_OF["SVCB_LEN"], a0=1)
    add("svcb_param_header_cut", over(answer(SVCB, b"\x00\x01\x00" + b"\x00\x01\x00")), err=E_OF["SVCB_TRUNC"])
    add("svcb_param_value_cut", over(answer(SVCB, b"\x00\x01\x00" + struct.pack(">HH", 1, 3) + b"h2")), err=E_OF["SVCB_TRUNC"])
    add("rrsig_small", over(answer(RRSIG, bytes(17))), err=E_OF["RRSIG"])
    add("rrsig_no_signer", over(answer(RRSIG, bytes(18))), err=E_OF["OFFHIGH"])
    add("dnskey_small", over(answer(DNSKEY, bytes(3))), err=E_OF["DNSKEY"])
    return c, E


E_OF = dict(zip("SHORT MAXREC OFFHIGH LONG INVIDX PTRHIGH RANGE Q40 Q80 QSMALL RSMALL RLEN CHARSTR SOA MX URI SRV NAPTR "
                "NF_MISS NF_TRUNC NS_MISS NS_TRUNC NR_MISS NR_TRUNC OPT_LEN OPT_MAL OPT_IMPL SVCB_LEN SVCB_TRUNC RRSIG "
                "DNSKEY".split(), range(90, 121)))


def layers17():
    """Ethernet, 13 Dot1Q tags, IPv4, UDP: 16 layers in front of the message; and one tag more."""
    tags = lambda n: MAC + b"".join(b"\x81\x00" + b"\x00\x05" for _ in range(n)) + b"\x08\x00"  # noqa: E731
    m = ip4(udp(hdr(1) + QEX, 50004, 53), 17)
    return tags(13) + m, tags(14) + m


def fuzz_packets(seed, n):
    """The cases' packets, four in ten as they are, the rest with one to three
    bytes of the message changed or the packet cut short (the frame and its
    length fields stay: the slice shrinks with the capture)."""
    rnd = random.Random(seed)
    base = [p for _, p in quirk_cases()[0]]
    out = []
    for _ in range(n):
        pkt = bytearray(rnd.choice(base))
        r = rnd.random()
        if r < 0.4 or len(pkt) <= 42:
            pass
        elif r < 0.85:
            for _ in range(rnd.randrange(1, 4)):
                pkt[rnd.randrange(42, len(pkt))] = rnd.choice([0, 1, 0xc0, 0x0c, 0x40, 0x80, 0xff, rnd.randrange(256)])
        else:
            pkt = pkt[:rnd.randrange(43, len(pkt) + 1)]
        out.append(bytes(pkt))
    return out


FUZZ_SEED = 20261022
FUZZ_N = 2048
