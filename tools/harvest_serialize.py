#!/usr/bin/env python3
"""Harvest the reference's own serialization pins as data into
tests/golden/serialize_vectors.json. Reads the reference source as text only;
nothing of it is executed.

  roundtrip   the packets testSerialization / testSerializationWithOpts assert to
              re-serialize to themselves (layers/decode_test.go:491, :532-547,
              the nine sctpPackets of :575-682, which are Ethernet + IPv4 + a
              verbatim tail here, :1363), with the option sets each is asserted under
  checksums   layers/tcpip_test.go:15-19 with the struct values of :21-56: the UDP
              checksums SerializeLayers computes with FixLengths and
              ComputeChecksums. ipv6UDPChecksumJumbogram is left out: the
              reference reaches it by inserting a HopByHop header
              (addIPv6JumboOption), which this project does not build.
  zero_udp    layers/udp_test.go:380-408: a computed checksum of 0 is written as 0xffff
  tcp_padding layers/tcp_test.go:55-70: one No-op option pads to 32 bits under FixLengths
  hopbyhop0   layers/ip6_test.go:96-134: testPacketIPv6HopByHop0 out of FixLengths

  python tools/harvest_serialize.py <root of the reference's source tree>"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "serialize_vectors.json")
ALL4 = [[0, 0], [1, 0], [0, 1], [1, 1]]  # [FixLengths, ComputeChecksums], testSerialization's order


def byte_array(src, name, decl="var %s = \\[\\]byte\\{"):
    m = re.search((decl % name) + r"(.*?)\n\s*\}", src, re.S)
    assert m, name
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", body))


def const(src, name):
    m = re.search(r"%s\s*=\s*uint16\((0x[0-9a-fA-F]+)\)" % name, src)
    assert m, name
    return int(m.group(1), 16)


def ip_of(src, func, field):
    m = re.search(r"func %s\(.*?\n\}" % func, src, re.S)
    assert m, func
    a = re.search(r"%s = net\.ParseIP\(\"([^\"]+)\"\)" % field, m.group(0))
    assert a, field
    return a.group(1)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    rd = lambda p: open(os.path.join(root, p)).read()
    dec, tcpip, udp, tcp, ip6 = (rd("layers/" + f) for f in
                                 ("decode_test.go", "tcpip_test.go", "udp_test.go", "tcp_test.go", "ip6_test.go"))
    out = {"roundtrip": [], "checksums": [], "left_out": []}
    assert "testSerialization(t, p, testSimpleTCPPacket)" in dec and "testSerialization(t, p, smallPacket)" in dec
    assert "testSerializationWithOpts(t, p, testPacketIPv4Fragmented, gopacket.SerializeOptions{FixLengths: true, " \
           "ComputeChecksums: true})" in dec
    out["roundtrip"].append({"name": "testSimpleTCPPacket", "source": "layers/decode_test.go:23,491", "first": 17,
                             "packet": byte_array(dec, "testSimpleTCPPacket").hex(), "opts": ALL4})
    out["roundtrip"].append({"name": "smallPacket", "source": "layers/decode_test.go:532-547", "first": 17,
                             "packet": byte_array(dec, "smallPacket", "%s := \\[\\]byte\\{").hex(), "opts": ALL4})
    out["roundtrip"].append({"name": "testPacketIPv4Fragmented", "source": "layers/decode_test.go:1349,1363",
                             "first": 17, "packet": byte_array(dec, "testPacketIPv4Fragmented").hex(),
                             "opts": [[1, 1]]})
    m = re.search(r"sctpPackets := \[\]\[\]byte\{(.*?)\n\t\t\}\}", dec, re.S)
    assert m, "sctpPackets"
    sctp = re.findall(r"\[\]byte\{([^}]*)", m.group(1))
    assert len(sctp) == 9 and "testSerializationWithOpts(t, p, data, gopacket.SerializeOptions{FixLengths: true, " \
        "ComputeChecksums: true})" in dec
    for i, body in enumerate(sctp):
        body = re.sub(r"//[^\n]*", "", body)
        out["roundtrip"].append({"name": "sctpPackets[%d]" % i, "source": "layers/decode_test.go:575-682", "first": 17,
                                 "packet": bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", body)).hex(),
                                 "opts": [[1, 1]]})
    v4 = {"src": ip_of(tcpip, "createIPv4ChecksumTestLayer", "ip4.SrcIP"),
          "dst": ip_of(tcpip, "createIPv4ChecksumTestLayer", "ip4.DstIP"), "ttl": 64}
    v6 = {"src": ip_of(tcpip, "createIPv6ChecksumTestLayer", "ip6.SrcIP"),
          "dst": ip_of(tcpip, "createIPv6ChecksumTestLayer", "ip6.DstIP"), "hop_limit": 64}
    ports = [int(re.search(r"udp\.SrcPort = UDPPort\((\d+)\)", tcpip).group(1)),
             int(re.search(r"udp\.DstPort = UDPPort\((\d+)\)", tcpip).group(1))]
    out["checksums"].append({"name": "ipv4UDPChecksum", "source": "layers/tcpip_test.go:16,58-93", "ip4": v4,
                             "ports": ports, "want": const(tcpip, "ipv4UDPChecksum")})
    out["checksums"].append({"name": "ipv6UDPChecksumWithIPv6DstOpts", "source": "layers/tcpip_test.go:17,95-135",
                             "ip6": v6, "ports": ports, "destination": "1100010400000000",
                             "want": const(tcpip, "ipv6UDPChecksumWithIPv6DstOpts")})
    out["left_out"].append({"source": "layers/tcpip_test.go:18,137-186 ipv6UDPChecksumJumbogram",
                            "want": const(tcpip, "ipv6UDPChecksumJumbogram"),
                            "reason": "the HopByHop header and its jumbo option are inserted by addIPv6JumboOption "
                                      "(GPK_SER_EJUMBOADD); a source packet that already has them is a jumbogram, "
                                      "whose HopByHop the reference's decode leaves in the payload"})
    z = re.search(r"func TestZeroChecksum.*?\n\}", udp, re.S).group(0)
    out["zero_udp"] = {"source": "layers/udp_test.go:380-408",
                       "src": re.search(r"SrcIP:\s+net\.ParseIP\(\"([^\"]+)\"\)", z).group(1),
                       "dst": re.search(r"DstIP:\s+net\.ParseIP\(\"([^\"]+)\"\)", z).group(1),
                       "ports": [int(re.search(r"SrcPort: (\d+)", z).group(1)), int(re.search(r"DstPort: (\d+)", z).group(1))],
                       "want": 0xFFFF}
    assert "TCPOptionKindNop" in re.search(r"func TestTCPSerializePadding.*?\n\}", tcp, re.S).group(0)
    out["tcp_padding"] = {"source": "layers/tcp_test.go:55-70", "options": "01", "multiple_of": 4}
    out["hopbyhop0"] = {"source": "layers/ip6_test.go:96-134", "first": 21, "opts": [[1, 0]],
                        "packet": byte_array(ip6, "testPacketIPv6HopByHop0").hex()}
    json.dump(out, open(OUT, "w"), indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
