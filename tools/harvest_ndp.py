#!/usr/bin/env python3
"""Harvest the NDP and MLD pins of the reference's tests into
tests/golden/ndp_vectors.json (data only: packet bytes and the values the Go
tests assert or describe, read from the test files as text).

    python tools/harvest_ndp.py /path/to/gopacket

  layers/icmp6msg_test.go       the RouterAdvertisement and NeighborSolicitation packets (checkLayers)
  layers/icmp6NDflags_test.go   a Neighbor and a Router Advertisement with the flag helpers' asserted values
  layers/icmp6hopbyhop_test.go  icmp6HopByHopData (checkLayers ends at ICMPv6: what the default decoder gives)
  layers/mldv1_test.go          Query, Report and Done (checkLayers; the dissection in the comment above each)
  layers/mldv2_test.go          Query and Report (the same)

A vector: name, source, hex (an Ethernet frame) and expect: "layers" (the
test's checkLayers list) where the test has one, "flags" (helper name ->
asserted value) for the NDflags pair, and "dissection": the fields the comment
above an MLD packet lists (Maximum Response Code, the multicast addresses in
order, QQIC, S, QRV, Number of Sources, Number of Multicast Address Records, the
record types).
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = json.load(open(os.path.join(ROOT, "gopacket_amd", "registry_gen.json")))
LT = {}
for _k, _v in REG["layer_type_names"].items():
    LT.setdefault(_v.replace(" ", ""), int(_k))


def byte_array(src, name):
    m = re.search(r"var %s = \[\]byte\{(.*?)\n\}" % re.escape(name), src, re.S)
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", body))


def layer_list(src, var):
    m = re.search(r"NewPacket\(%s,.*?checkLayers\(p, \[\]gopacket\.LayerType\{(.*?)\}, t\)" % re.escape(var), src, re.S)
    return [LT[n] for n in re.findall(r"LayerType(\w+)", m.group(1))]


def comment_above(src, var):
    """The comment block that ends at `var NAME`, as text."""
    head = src[:src.index("var %s = " % var)]
    lines = []
    for line in reversed(head.rstrip("\n").split("\n")):
        if not line.startswith("//"):
            break
        lines.append(line[2:].strip())
    return "\n".join(reversed(lines))


def dissection(text):
    """The ICMPv6 part of a Wireshark dissection in a comment."""
    text = text[text.index("Internet Control Message Protocol v6"):]
    d = {}

    def num(key, pattern):
        m = re.search(pattern, text)
        if m:
            d[key] = int(m.group(1))
    num("Type", r"Type: [^\n]*\((\d+)\)")
    num("MaximumResponseCode", r"Maximum Response Code: (\d+)")
    num("QQIC", r"QQIC[^\n]*: (\d+)")
    num("QRV", r"QRV[^\n]*: (\d+)")
    num("NumberOfSources", r"\nNumber of Sources: (\d+)")
    num("NumberOfMulticastAddressRecords", r"Number of Multicast Address Records: (\d+)")
    m = re.search(r"Suppress Router-Side Processing: (\w+)", text)
    if m:
        d["S"] = m.group(1) != "False"
    d["MulticastAddresses"] = re.findall(r"\nMulticast Address: (\S+)", "\n" + text)
    d["RecordTypes"] = [int(x) for x in re.findall(r"Record Type: \w+ \((\d+)\)", text)]
    return d


def asserted_flags(src, func, var):
    """{helper: value} from `if [!]var.Helper() { t.Errorf(...) }` of one test function."""
    body = src[src.index("func %s(" % func):]
    body = body[:body.index("\n}\n")]
    return {name: bool(neg) for neg, name in re.findall(r"if (!?)%s\.(\w+)\(\) \{" % re.escape(var), body)}


def main(ref):
    vectors = []

    def read(name):
        return open(os.path.join(ref, "layers", name)).read()

    def add(name, source, frame, **expect):
        vectors.append(dict(name=name, source="layers/" + source, hex=frame.hex(), expect=expect))

    src = read("icmp6msg_test.go")
    for var in ("testPacketICMPv6RouterAdvertisement", "testPacketICMPv6NeighborSolicitation"):
        add(var, "icmp6msg_test.go", byte_array(src, var), layers=layer_list(src, var))
    src = read("icmp6NDflags_test.go")
    add("icmp6NeighborAnnouncementData", "icmp6NDflags_test.go", byte_array(src, "icmp6NeighborAnnouncementData"),
        flags=asserted_flags(src, "TestPacketICMPv6NeighborAnnouncementFlags", "icmpNeighAdvLayer"))
    add("icmp6RouterAdvertisementData", "icmp6NDflags_test.go", byte_array(src, "icmp6RouterAdvertisementData"),
        flags=asserted_flags(src, "TestPacketICMPv6RouterAnnouncementFlags", "icmpRouterAdvLayer"))
    src = read("icmp6hopbyhop_test.go")
    add("icmp6HopByHopData", "icmp6hopbyhop_test.go", byte_array(src, "icmp6HopByHopData"),
        layers=layer_list(src, "icmp6HopByHopData"))
    for name, variables in (("mldv1_test.go", ("testPacketMulticastListenerQueryMessageV1",
                                               "testPacketMulticastListenerReportMessageV1",
                                               "testPacketMulticastListenerDoneMessageV1")),
                            ("mldv2_test.go", ("testPacketMulticastListenerQueryMessageV2",
                                               "testPacketMulticastListenerReportMessageV2"))):
        src = read(name)
        for var in variables:
            add(var, name, byte_array(src, var), layers=layer_list(src, var),
                dissection=dissection(comment_above(src, var)))
    out = os.path.join(ROOT, "tests", "golden", "ndp_vectors.json")
    with open(out, "w") as f:
        json.dump(dict(vectors=vectors), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d vectors -> %s" % (len(vectors), out))


if __name__ == "__main__":
    main(sys.argv[1])
