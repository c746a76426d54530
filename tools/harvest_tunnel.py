#!/usr/bin/env python3
"""Harvest the tunnel pins of the reference's tests into
tests/golden/tunnel_vectors.json (data only: packet bytes and expected field
values, read from the Go test files as text).

    python tools/harvest_tunnel.py /path/to/gopacket

  layers/vxlan_test.go   TestPacketVXLAN
  layers/geneve_test.go  TestDecodeGeneve1-4
  layers/gre_test.go     TestPacketGRE, TestPacketEthernetOverGRE,
                         TestGREDecodeFromBytesTruncatedOptionalFields, TestGREChecksum

A vector: name, hex (the packet), first (LayerType of the packet's first
decodable layer) and skip (bytes before it: the Linux SLL header of
TestDecodeGeneve1 has no decoder here), layers (the test's checkLayers list),
and the expected struct fields with Contents / Payload as [start, end) of the
packet. TestGREChecksum serializes its packets; they are rebuilt here from the
test's field values (FixLengths, ComputeChecksums), and the pin is the GRE
checksum the test expects. The truncated GRE headers are bare headers
(DecodeFromBytes input); the tests wrap them in Ethernet / IPv4.
"""
import json
import os
import re
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = json.load(open(os.path.join(ROOT, "gopacket_amd", "registry_gen.json")))
LT = {}
for _k, _v in REG["layer_type_names"].items():
    LT.setdefault(_v.replace(" ", ""), int(_k))  # "Linux SLL" is LayerTypeLinuxSLL
ETHERTYPES = {"EthernetTypeTransparentEthernetBridging": 0x6558, "EthernetTypeIPv4": 0x0800}


def strip_comments(s):
    return re.sub(r"//[^\n]*", "", s)


def byte_array(src, name):
    m = re.search(r"var %s = \[\]byte\{(.*?)\n\}" % re.escape(name), src, re.S)
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", strip_comments(m.group(1))))


def func_body(src, name):
    m = re.search(r"func %s\(t \*testing\.T\) \{(.*?)\n\}\n" % re.escape(name), src, re.S)
    return m.group(1)


def layer_list(body):
    m = re.search(r"checkLayers\(p, \[\]gopacket\.LayerType\{(.*?)\}, t\)", body, re.S)
    names = re.findall(r"LayerType(\w+)", m.group(1))
    return [LT[n] for n in names]


def num(expr):
    return int(eval(expr, {"__builtins__": {}}))  # "0xa", "124 + 4"


def span(expr, total):
    m = re.search(r"\[(\d*):(\d*)\]", expr)
    return [int(m.group(1) or 0), int(m.group(2)) if m.group(2) else total]


def bools(block, names):
    return {n: re.search(r"%s:\s+(true|false)" % n, block).group(1) == "true" for n in names
            if re.search(r"%s:\s+(true|false)" % n, block)}


def ip4_checksum(h):
    s = sum(struct.unpack(">10H", h))
    while s > 0xffff:
        s = (s >> 16) + (s & 0xffff)
    return ~s & 0xffff


def csum(data):
    if len(data) & 1:
        data += b"\x00"
    s = sum(struct.unpack(">%dH" % (len(data) // 2), data))
    while s > 0xffff:
        s = (s >> 16) + (s & 0xffff)
    return ~s & 0xffff


def ip4(src, dst, proto, ttl, ident, flags, payload):
    h = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(payload), ident, flags << 13, ttl, proto, 0) + bytes(src) + bytes(dst)
    return h[:10] + struct.pack(">H", ip4_checksum(h)) + h[12:] + payload


def gre_checksum_vectors(src):
    """TestGREChecksum: rebuild what SerializeLayers(FixLengths, ComputeChecksums) writes."""
    m = re.search(r"var testGREChecksum = map\[uint16\]\[\]gopacket\.SerializableLayer\{(.*?)\n\}\n", src, re.S)
    out = []
    for key, block in re.findall(r"\n\t(0x[0-9a-f]{4}): \{(.*?)\n\t\},", m.group(1), re.S):
        ips = [[int(x) for x in g.split(",")] for g in re.findall(r"net\.IP\{([\d, ]+)\}", block)]
        macs = [bytes(int(x, 16) for x in re.findall(r"0x([0-9a-f]{2})", g))
                for g in re.findall(r"net\.HardwareAddr\{(.*?)\}", block)]
        ip_blocks = re.findall(r"&IPv4\{(.*?)\n\t\t\},", block, re.S)
        payload = bytes(int(x, 16) for x in re.findall(
            r"0x([0-9a-f]{2})", re.search(r"gopacket\.Payload\{(.*?)\n\t\t\},", block, re.S).group(1)))

        def ipf(b, name, default=0):
            mm = re.search(r"%s:\s+(\d+)" % name, b)
            return int(mm.group(1)) if mm else default
        inner_b = ip_blocks[1]
        if "ICMPv4{" in block:
            ib = re.search(r"&ICMPv4\{(.*?)\n\t\t\},", block, re.S).group(1)
            l4 = struct.pack(">BBHHH", 8, 0, 0, ipf(ib, "Id"), ipf(ib, "Seq")) + payload
            l4 = l4[:2] + struct.pack(">H", csum(l4)) + l4[4:]
            proto = 1
        else:
            ub = re.search(r"&UDP\{(.*?)\n\t\t\},", block, re.S).group(1)
            l4 = struct.pack(">HHHH", ipf(ub, "SrcPort"), ipf(ub, "DstPort"), 8 + len(payload), 0) + payload
            pseudo = bytes(ips[2]) + bytes(ips[3]) + struct.pack(">HH", 17, len(l4))
            l4 = l4[:6] + struct.pack(">H", csum(pseudo + l4)) + l4[8:]
            proto = 17
        flags = 2 if "IPv4DontFragment" in inner_b else 0
        inner = ip4(ips[2], ips[3], proto, ipf(inner_b, "TTL"), ipf(inner_b, "Id"), flags, l4)
        gre = struct.pack(">BBHHH", 0x80, 0, 0x0800, 0, 0) + inner
        gre = gre[:4] + struct.pack(">H", csum(gre)) + gre[6:]
        ob = ip_blocks[0]
        pkt = macs[1] + macs[0] + struct.pack(">H", 0x0800) + ip4(ips[0], ips[1], 47, ipf(ob, "TTL"), ipf(ob, "Id"), 0, gre)
        out.append(dict(name="TestGREChecksum_%s" % key, source="layers/gre_test.go", hex=pkt.hex(), first=17, skip=0,
                        kind="GRE", expect=dict(Checksum=int(key, 16), ChecksumPresent=True, Protocol=0x0800,
                                                Contents=[34, 42], Payload=[42, len(pkt)], Valid=True)))
    return out


def main(ref):
    vectors = []
    src = open(os.path.join(ref, "layers", "vxlan_test.go")).read()
    pkt = byte_array(src, "testPacketVXLAN")
    body = func_body(src, "TestPacketVXLAN")
    want = re.search(r"want := &VXLAN\{(.*?)\n\t\t\}", body, re.S).group(1)
    contents = bytes(int(x, 16) for x in re.findall(r"0x([0-9a-f]{2})", re.search(r"Contents: \[\]byte\{(.*?)\}", want, re.S).group(1)))
    at = pkt.index(contents + pkt[50:60])
    e = dict(Contents=[at, at + len(contents)], Payload=[at + len(contents), len(pkt)],
             VNI=num(re.search(r"VNI:\s+(\w+)", want).group(1)),
             GBPGroupPolicyID=num(re.search(r"GBPGroupPolicyID:\s+(\w+)", want).group(1)))
    e.update(bools(want, ["ValidIDFlag", "GBPExtension", "GBPApplied", "GBPDontLearn"]))
    vectors.append(dict(name="TestPacketVXLAN", source="layers/vxlan_test.go", hex=pkt.hex(), first=17, skip=0,
                        kind="VXLAN", layers=layer_list(body), expect=e))

    src = open(os.path.join(ref, "layers", "geneve_test.go")).read()
    maxopt = byte_array(src, "testMaxSizeOption")
    for k in (1, 2, 3, 4):
        name = "testPacketGeneve%d" % k
        pkt = byte_array(src, name)
        body = func_body(src, "TestDecodeGeneve%d" % k)
        want = re.search(r"want := &Geneve\{(.*?)\n\t\t\}\n", body, re.S).group(1)
        e = dict(Contents=span(re.search(r"Contents: (\S+),", want).group(1), len(pkt)),
                 Payload=span(re.search(r"Payload:\s+(\S+),", want).group(1), len(pkt)),
                 Version=num(re.search(r"Version:\s+(\w+)", want).group(1)),
                 OptionsLength=num(re.search(r"OptionsLength:\s+([^,]+),", want).group(1)),
                 Protocol=ETHERTYPES[re.search(r"Protocol:\s+(\w+)", want).group(1)],
                 VNI=num(re.search(r"VNI:\s+(\w+)", want).group(1)), Options=[])
        e.update(bools(want, ["OAMPacket", "CriticalOption"]))
        for ob in re.findall(r"\n\t\t\t\t\{(.*?)\n\t\t\t\t\},", want, re.S):
            dm = re.search(r"Data:\s+(.*)", ob, re.S).group(1)
            data = maxopt if "testMaxSizeOption" in dm else bytes(num(x) for x in re.search(r"\{(.*?)\}", dm).group(1).split(","))
            e["Options"].append(dict(Class=num(re.search(r"Class:\s+(\w+)", ob).group(1)),
                                     Type=num(re.search(r"Type:\s+(\w+)", ob).group(1)),
                                     Length=num(re.search(r"Length:\s+([^,]+),", ob).group(1)), Data=data.hex()))
        sll = "LinkTypeLinuxSLL" in body
        vectors.append(dict(name="TestDecodeGeneve%d" % k, source="layers/geneve_test.go", hex=pkt.hex(),
                            first=20 if sll else 17, skip=16 if sll else 0, kind="Geneve", layers=layer_list(body),
                            expect=e))

    src = open(os.path.join(ref, "layers", "gre_test.go")).read()
    for test, var in (("TestPacketGRE", "testPacketGRE"), ("TestPacketEthernetOverGRE", "testPacketEthernetOverGRE")):
        pkt = byte_array(src, var)
        body = func_body(src, test)
        want = re.search(r"want := &GRE\{(.*?)\n\t\t\}\n", body, re.S).group(1)
        sp = re.findall(r"%s(\[\d*:\d*\])" % var, want)
        e = dict(Contents=span(sp[0], len(pkt)), Payload=span(sp[1], len(pkt)),
                 Protocol=ETHERTYPES[re.search(r"Protocol:\s+(\w+)", want).group(1)], ChecksumPresent=False,
                 Checksum=0, Key=0, Seq=0, Ack=0)
        vectors.append(dict(name=test, source="layers/gre_test.go", hex=pkt.hex(), first=17, skip=0, kind="GRE",
                            layers=layer_list(body), expect=e))
    body = func_body(src, "TestGREDecodeFromBytesTruncatedOptionalFields")
    for nm, data in re.findall(r'name: "([^"]+)",\s+data: \[\]byte\{(.*?)\},\n\t\t\}', body, re.S):
        raw = bytes(int(x, 16) for x in re.findall(r"0x([0-9a-f]{2})", data))
        vectors.append(dict(name="TestGRETruncated_" + nm.replace(" ", "_"), source="layers/gre_test.go", hex=raw.hex(),
                            kind="GRE", bare_header=True, expect=dict(error=True, truncated=True)))
    vectors += gre_checksum_vectors(src)
    out = os.path.join(ROOT, "tests", "golden", "tunnel_vectors.json")
    with open(out, "w") as f:
        json.dump(dict(vectors=vectors), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d vectors -> %s" % (len(vectors), out))


if __name__ == "__main__":
    main(sys.argv[1])
