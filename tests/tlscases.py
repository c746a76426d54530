"""Hand-built TLS messages: one per error text of include/gpk_tls.h at its
boundary, one per quirk of its rules, and the seeded mutation
corpus of the TLS tests.

Every case is (name, packet bytes). The expected arrays come from
tls_model.py; EXPECT also carries, by hand from the reference's source, each
case's error code and arguments (0: it decodes), its status, and for some the
record kinds, the handshake forms and the server names, so the model is
checked too. A case without an expectation is not a candidate.

The parser sends TCP port 8443 to LayerTypeTLS (gpk_parser_set_tcp_port): the
table-edited port. The message of over() starts at packet offset 54.
"""
import random
import struct

from tunnelcases import MAC, eth, dot1q, ip4, ip6, tcp, vxlan, over_udp, VX  # noqa: F401

PARSER = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"],
              tcp_port={8443: 140})
PARSER_IGNORE = dict(PARSER, ignore_unsupported=True)
PARSER_NOPAYLOAD = dict(PARSER, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP"])
CCS, ALERT, HS, APP = 20, 21, 22, 23
E_OF = dict(zip("REC_SHORT REC_TYPE LEN CCS ALERT HS_SHORT HS_TYPE CH_SHORT CH_SESSION CH_CIPHERS CH_COMPRESSION "
                "CH_EXTENSIONS".split(), range(121, 133)), PANIC=4)
KNOWN_HANDSHAKE_TYPES = (0, 1, 2, 3, 11, 12, 13, 14, 15, 16, 20)
HS_ENC, HS_HELLO, HS_KEY = 1, 2, 3
AT = 54


def rec(ct, body=b"", ver=0x0303, length=None):
    return struct.pack(">BHH", ct, ver, len(body) if length is None else length) + body


def over(msg, sport=40000, dport=443):
    return eth(ip4(tcp(msg, sport, dport), 6))


def ext(typ, data=b"", length=None):
    return struct.pack(">HH", typ, len(data) if length is None else length) + data


def sni_ext(host=b"example.com", list_len=None, entry_type=0, host_len=None, length=None):
    body = struct.pack(">HBH", len(host) + 3 if list_len is None else list_len, entry_type,
                       len(host) if host_len is None else host_len) + host
    return ext(0, body, length)


ALPN = ext(16, b"\x00\x03\x02h2")
GROUPS = ext(10, b"\x00\x02\x00\x1d")


def hello_tail(exts=None, sid=b"", ciphers=b"\x13\x01\x13\x02", comp=b"\x00", ext_len=None):
    """A ClientHello from its session ID length on."""
    exts = sni_ext() + ALPN if exts is None else exts
    return (bytes([len(sid)]) + sid + struct.pack(">H", len(ciphers)) + ciphers + bytes([len(comp)]) + comp +
            struct.pack(">H", len(exts) if ext_len is None else ext_len) + exts)


def hello(exts=None, be24=None, **kw):
    """A ClientHello handshake message: type, 24-bit length, version, random, then hello_tail."""
    rest = struct.pack(">H", 0x0303) + bytes(range(32)) + hello_tail(exts, **kw)
    n = len(rest) if be24 is None else be24
    return b"\x01" + n.to_bytes(3, "big") + rest


def hs_body(typ, n, be24=None):
    """A handshake body of n >= 4 bytes: type, 24-bit length (default n - 4), filler."""
    return bytes([typ]) + (n - 4 if be24 is None else be24).to_bytes(3, "big") + bytes((0x40 + k) & 0xFF for k in range(n - 4))


def cut_hello(k, **kw):
    """A handshake record whose body is the first k bytes of a ClientHello, its
    24-bit length set so that the record counts as plaintext: at the end of a
    packet the ClientHello has exactly k bytes to read."""
    return rec(HS, hs_body(1, 4, k - 4)[:4] + hello(**kw)[4:k])


def spill(tail):
    """A 4-byte plaintext handshake record of type 1 and an Application Data
    record behind it: the ClientHello reads on through the second record's
    header (its version and the start of its random) into its body, where
    `tail` (hello_tail) lies at body offset 38."""
    return rec(HS, b"\x01\x00\x00\x00") + rec(APP, bytes(29) + tail)


def quirk_cases():
    c = []
    E = {}

    def add(nm, pkt, **expect):
        c.append((nm, pkt))
        E[nm] = expect
    T = dict(status=1)  # Truncated
    # ---- records (tls.go:130-194)
    add("appdata_1", over(rec(APP, bytes(range(32)))), err=0, kinds=[APP])
    add("appdata_2", over(rec(APP, bytes(32)) + rec(APP, bytes(range(7)), ver=0x0301)), err=0, kinds=[APP, APP])
    add("appdata_from_server", over(rec(APP, b"reply"), 443, 50000), err=0, kinds=[APP])  # the source port is 443
    add("four_kinds", over(rec(HS, hs_body(16, 20)) + rec(CCS, b"\x01") + rec(ALERT, b"\x02\x28") + rec(APP, b"data") +
                           rec(HS, bytes(range(100, 140)))), err=0, kinds=[HS, CCS, ALERT, APP, HS],
        hs=[HS_KEY, 0, 0, 0, HS_ENC])
    add("appdata_300_empty", over(rec(APP) * 300), err=0, kinds=[APP] * 300)
    add("record_exactly_5", over(rec(APP)), err=0, kinds=[APP])
    add("record_short_4", over(rec(APP)[:4]), err=E_OF["REC_SHORT"], **T)
    add("record_short_1", over(b"\x17"), err=E_OF["REC_SHORT"], **T)
    add("second_record_short_4", over(rec(APP, b"abc") + rec(APP)[:4]), err=E_OF["REC_SHORT"], **T)
    add("record_type_19", over(rec(19, b"x")), err=E_OF["REC_TYPE"])
    add("record_type_24", over(rec(24, b"x")), err=E_OF["REC_TYPE"])
    add("record_type_before_length", over(rec(0x50, b"", length=0xFFFF)), err=E_OF["REC_TYPE"])  # not the length error
    add("length_one_short", over(rec(APP, bytes(10), length=11)), err=E_OF["LEN"], **T)
    add("length_ffff", over(rec(APP, bytes(10), length=0xFFFF)), err=E_OF["LEN"], **T)
    add("second_length_one_short", over(rec(CCS, b"\x01") + rec(HS, bytes(40), length=41)), err=E_OF["LEN"], **T)
    # ---- ChangeCipherSpec (tls_cipherspec.go:37-54)
    add("ccs_message_1", over(rec(CCS, b"\x01")), err=0, kinds=[CCS], v0=[1])
    add("ccs_message_2_is_255", over(rec(CCS, b"\x02")), err=0, kinds=[CCS], v0=[255])
    add("ccs_message_0_is_255", over(rec(CCS, b"\x00")), err=0, kinds=[CCS], v0=[255])
    add("ccs_length_0", over(rec(CCS)), err=E_OF["CCS"], **T)
    add("ccs_length_2", over(rec(CCS, b"\x01\x01")), err=E_OF["CCS"], **T)
    # ---- Alert (tls_alert.go:74-95)
    add("alert_length_0", over(rec(ALERT)), err=E_OF["ALERT"], **T)
    add("alert_length_1", over(rec(ALERT, b"\x01")), err=E_OF["ALERT"], **T)
    add("alert_warning_close_notify", over(rec(ALERT, b"\x01\x00")), err=0, kinds=[ALERT], v0=[1], v1=[0])
    add("alert_fatal_handshake_failure", over(rec(ALERT, b"\x02\x28")), err=0, kinds=[ALERT], v0=[2], v1=[40])
    add("alert_length_3_is_encrypted", over(rec(ALERT, b"\x02\x28\x00")), err=0, kinds=[ALERT], v0=[255], v1=[255])
    add("alert_length_32_is_encrypted", over(rec(ALERT, bytes(range(32)))), err=0, kinds=[ALERT], v0=[255], v1=[255])
    # ---- Handshake (tls_handshake.go:198-251)
    add("handshake_length_0", over(rec(HS)), err=E_OF["HS_SHORT"], **T)
    add("handshake_length_15_unknown_type", over(rec(HS, hs_body(99, 15))), err=E_OF["HS_TYPE"])  # below 16: plaintext
    add("handshake_length_16_unknown_type", over(rec(HS, hs_body(99, 16))), err=0, kinds=[HS], hs=[HS_ENC])
    add("handshake_be24_not_length_minus_4", over(rec(HS, hs_body(2, 16, 13))), err=0, kinds=[HS], hs=[HS_ENC])
    add("handshake_be24_above_length", over(rec(HS, hs_body(2, 16, 0xFFFFFF))), err=0, kinds=[HS], hs=[HS_ENC])
    add("handshake_be24_is_length_minus_4_known_type", over(rec(HS, hs_body(2, 20, 16))), err=E_OF["HS_TYPE"])
    add("plaintext_server_hello", over(rec(HS, hs_body(2, 60))), err=E_OF["HS_TYPE"])
    add("plaintext_certificate_after_appdata", over(rec(APP, b"x") + rec(HS, hs_body(11, 200))), err=E_OF["HS_TYPE"])
    for t in KNOWN_HANDSHAKE_TYPES:  # 16 bytes whose 24-bit length is 12: plaintext for every known type
        if t == 1:  # a ClientHello with 16 bytes to read
            add("known_type_1_at_16", over(rec(HS, hs_body(1, 16))), err=E_OF["CH_SHORT"], **T)
        elif t == 16:
            add("known_type_16_at_16", over(rec(HS, hs_body(16, 16))), err=0, kinds=[HS], hs=[HS_KEY])
        else:
            add("known_type_%d_at_16" % t, over(rec(HS, hs_body(t, 16))), err=E_OF["HS_TYPE"])
    add("client_key_exchange_4_bytes", over(rec(HS, b"\x10\x00\x00\x00")), err=0, kinds=[HS], hs=[HS_KEY])
    add("client_key_exchange_1_byte", over(rec(HS, b"\x10")), err=0, kinds=[HS], hs=[HS_KEY])
    # ---- ClientHello (tls_handshake.go:104-189)
    add("hello_with_sni", over(rec(HS, hello(), ver=0x0301)), err=0, kinds=[HS], hs=[HS_HELLO], sni=[b"example.com"])
    add("hello_then_appdata", over(rec(HS, hello(sni_ext(b"a.test"))) + rec(APP, b"early")), err=0, kinds=[HS, APP],
        sni=[b"a.test"])
    add("two_hellos", over(rec(HS, hello(sni_ext(b"one.test"))) + rec(HS, hello(sni_ext(b"two.test")))), err=0,
        kinds=[HS, HS], sni=[b"one.test", b"two.test"])
    full = len(hello(sid=b"\xaa\xbb\xcc\xdd", ciphers=b"\x13\x01", comp=b"\x00"))
    kw = dict(sid=b"\xaa\xbb\xcc\xdd", ciphers=b"\x13\x01", comp=b"\x00")
    # with a 4-byte session ID, 2 cipher bytes and 1 method: the checks want 39, 45, 48, 51 and 51 + extensions
    add("hello_38_bytes", over(cut_hello(38, **kw)), err=E_OF["CH_SHORT"], **T)
    add("hello_39_bytes", over(cut_hello(39, **kw)), err=E_OF["CH_SESSION"], **T)
    add("hello_44_bytes", over(cut_hello(44, **kw)), err=E_OF["CH_SESSION"], **T)
    add("hello_45_bytes", over(cut_hello(45, **kw)), err=E_OF["CH_CIPHERS"], **T)
    add("hello_47_bytes", over(cut_hello(47, **kw)), err=E_OF["CH_CIPHERS"], **T)
    add("hello_48_bytes", over(cut_hello(48, **kw)), err=E_OF["CH_COMPRESSION"], **T)
    add("hello_50_bytes", over(cut_hello(50, **kw)), err=E_OF["CH_COMPRESSION"], **T)
    add("hello_51_bytes", over(cut_hello(51, **kw)), err=E_OF["CH_EXTENSIONS"], **T)
    add("hello_one_byte_short", over(cut_hello(full - 1, **kw)), err=E_OF["CH_EXTENSIONS"], **T)
    add("hello_exact", over(cut_hello(full, **kw)), err=0, kinds=[HS], hs=[HS_HELLO], sni=[b"example.com"])
    add("hello_no_extensions_block", over(rec(HS, hello(b""))), err=0, kinds=[HS], hs=[HS_HELLO], sni=[None])
    add("hello_of_15_bytes", over(rec(HS, hello(be24=5)[:15])), err=E_OF["CH_SHORT"], **T)  # below 16: plaintext whatever its length field
    # the ClientHello reads past its record: into the next record, to the end of the packet
    add("hello_spills_into_next_record", over(spill(hello_tail(sni_ext(b"spill.test")))), err=0, kinds=[HS, APP],
        hs=[HS_HELLO, 0], sni=[b"spill.test"])
    add("hello_spill_ends_with_packet", over(spill(hello_tail(sni_ext(b"end.test") + GROUPS))), err=0, kinds=[HS, APP],
        sni=[b"end.test"])
    n = len(sni_ext(b"end.test") + GROUPS)
    add("hello_spill_one_byte_short", over(spill(hello_tail(sni_ext(b"end.test") + GROUPS, ext_len=n + 1))),
        err=E_OF["CH_EXTENSIONS"], **T)
    add("hello_spill_extensions_end_early", over(spill(hello_tail(sni_ext(b"end.test") + GROUPS, ext_len=n - 8) + b"xy")),
        err=0, kinds=[HS, APP], sni=[b"end.test"])  # the block ends in front of GROUPS: the walk ends with the SNI extension
    # ---- the extension walk and the SNI reads
    add("sni_absent", over(rec(HS, hello(ALPN + GROUPS))), err=0, sni=[None])
    add("sni_empty_list", over(rec(HS, hello(sni_ext(b"x.test", list_len=0)))), err=0, sni=[None])
    add("sni_entry_type_1", over(rec(HS, hello(sni_ext(b"x.test", entry_type=1)))), err=0, sni=[None])
    add("sni_empty_hostname", over(rec(HS, hello(sni_ext(b"") + ALPN))), err=0, sni=[b""])  # not nil: data[9:9]
    add("sni_empty_hostname_at_block_end", over(rec(HS, hello(sni_ext(b"")))), err=0, sni=[b""])  # len(data) is 9 > 8 + 0
    add("sni_twice_last_wins", over(rec(HS, hello(sni_ext(b"first.test") + ALPN + sni_ext(b"second.test")))), err=0,
        sni=[b"second.test"])
    add("sni_second_fails_first_stays", over(rec(HS, hello(sni_ext(b"first.test") + sni_ext(b"x", entry_type=7)))), err=0,
        sni=[b"first.test"])
    # the extension holds list length and entry type only; hostnameLength is the next extension's type, the
    # hostname its length and first data byte
    add("sni_reads_reach_into_next_extension", over(rec(HS, hello(ext(0, b"\x00\x05\x00") + ext(3, b"\xab\xcd")))), err=0,
        sni=[b"\x00\x02\xab"])
    add("sni_hostname_longer_than_extension", over(rec(HS, hello(sni_ext(b"abc", host_len=8) + ALPN))), err=0,
        sni=[b"abc" + ALPN[:5]])
    add("sni_hostname_longer_than_block", over(rec(HS, hello(sni_ext(b"abc", host_len=20) + ALPN))), err=0, sni=[None])
    add("sni_hostname_length_fff7", over(rec(HS, hello(sni_ext(b"abc", host_len=0xFFF7)))), err=0, sni=[None])
    add("sni_hostname_length_fff8_panics", over(rec(HS, hello(sni_ext(b"abc", host_len=0xFFF8)))), err=E_OF["PANIC"],
        a0=9, a1=1)
    add("sni_hostname_length_ffff_panics", over(rec(HS, hello(sni_ext(b"abc", host_len=0xFFFF)))), err=E_OF["PANIC"],
        a0=9, a1=8)
    add("sni_panic_after_good_records", over(rec(APP, b"x") + rec(HS, hello(sni_ext(b"", host_len=0xFFFA) + ALPN))),
        err=E_OF["PANIC"], a0=9, a1=3)
    add("extension_longer_than_rest_stops_the_walk", over(rec(HS, hello(ext(16, b"ab", length=200) + sni_ext(b"hidden.test")))),
        err=0, sni=[None])
    add("extension_length_ffff", over(rec(HS, hello(ext(16, b"ab", length=0xFFFF) + sni_ext(b"hidden.test")))), err=0,
        sni=[None])
    add("three_bytes_left_stop_the_walk", over(rec(HS, hello(sni_ext(b"kept.test") + b"\x00\x00\x00"))), err=0,
        sni=[b"kept.test"])
    add("sni_extension_of_6_bytes", over(rec(HS, hello(ext(0, b"\x00\x01")))), err=0, sni=[None])  # len(data) 6, not > 6
    add("sni_extension_of_8_bytes", over(rec(HS, hello(ext(0, b"\x00\x01\x00\x00")))), err=0, sni=[None])  # not > 8
    # ---- carriers and candidates
    add("registered_port_8443", over(rec(APP, b"on 8443"), dport=8443), err=0, kinds=[APP])
    add("over_ipv6", eth(ip6(tcp(rec(HS, hello(sni_ext(b"v6.test"))), dport=443), 6), 0x86dd), err=0, sni=[b"v6.test"])
    add("over_dot1q", MAC + b"\x81\x00" + dot1q(ip4(tcp(rec(APP, b"tagged"), dport=993), 6)), err=0, kinds=[APP])
    add("ldaps_port_636", over(rec(ALERT, b"\x01\x00"), dport=636), err=0, kinds=[ALERT])
    add("empty_payload_on_443", over(b""))                # not a candidate: the loop ends before the type is looked at
    add("plain_tcp_port_80", over(rec(APP, b"http?"), dport=80))
    add("udp_port_443", eth(ip4(struct.pack(">HHHH", 50000, 443, 8 + 10, 0) + rec(APP, b"quic?"), 17)))
    return c, E


def layers17():
    """Ethernet, 13 Dot1Q tags, IPv4, TCP: 16 layers in front of the message; and one tag more."""
    tags = lambda n: MAC + b"".join(b"\x81\x00" + b"\x00\x05" for _ in range(n)) + b"\x08\x00"  # noqa: E731
    m = ip4(tcp(rec(APP, b"deep"), dport=443), 6)
    return tags(13) + m, tags(14) + m


def fuzz_packets(seed, n):
    """The cases' packets (the 300-record one left out), half of them as they
    are, the rest with one to three bytes changed at the fields that steer the
    walk (a record header, the handshake header, the ClientHello's length
    fields and its extension headers) or anywhere in the message, or the
    packet cut short (the frame and its length fields stay: the slice shrinks
    with the capture)."""
    rnd = random.Random(seed)
    base = [p for nm, p in quirk_cases()[0] if nm != "appdata_300_empty" and p[12:14] == b"\x08\x00" and len(p) > AT]
    steer = list(range(AT, AT + 10)) + list(range(AT + 43, AT + 60))
    out = []
    for _ in range(n):
        pkt = bytearray(rnd.choice(base))
        r = rnd.random()
        if r < 0.5:
            pass
        elif r < 0.85:
            for _ in range(rnd.randrange(1, 4)):
                at = rnd.choice(steer) if rnd.random() < 0.6 else rnd.randrange(AT, len(pkt))
                if at < len(pkt):
                    pkt[at] = rnd.choice([0, 1, 2, 4, 5, 16, 20, 21, 22, 23, 0xff, 0xf8, rnd.randrange(256)])
        else:
            pkt = pkt[:rnd.randrange(AT + 1, len(pkt) + 1)]
        out.append(bytes(pkt))
    return out


FUZZ_SEED = 20261021
FUZZ_N = 3072
