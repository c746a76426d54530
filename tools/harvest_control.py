#!/usr/bin/env python3
"""Harvest the ICMPv4 / ICMPv6 / ARP pins of the reference's tests and captures
into tests/golden/control_vectors.json (data only: packet bytes, the field
values the Go tests assert, read from the test files as text, and the checksum
pin computed here).

    python tools/harvest_control.py /path/to/gopacket

  layers/decode_test.go          testICMP, testICMP6 (the tcpdump line above each names the message)
  layers/icmp6_test.go           testPacketICMPv6 (TypeCode, Checksum, Contents, Payload)
  layers/icmp6hopbyhop_test.go   icmp6HopByHopData (the ICMPv6 type behind a HopByHop header)
  layers/icmp6msg_test.go        the RouterAdvertisement and NeighborSolicitation packets
  pcap/*.pcap                    every Ethernet frame that carries ARP, ICMPv4 or ICMPv6

A vector: name, source, hex (an Ethernet frame), kind ("ICMPv4", "ICMPv6",
"ARP"), at (offset of the control header), and expect: the asserted fields where
a test asserts them, the test's checkLayers list after the network layers, and
the pin {"Valid", "Correct", "Actual"}: VerifyChecksum worked out here with
RFC 1071 arithmetic over the message (and the IPv6 pseudo-header), not with the
model under test. These are real captures with intact checksums, so Valid is
true for each; the harvest fails otherwise.
"""
import glob
import json
import os
import re
import struct
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


def ones_sum(data, start=0):
    if len(data) & 1:
        data += b"\x00"
    s = start + sum(struct.unpack(">%dH" % (len(data) // 2), data))
    while s > 0xffff:
        s = (s >> 16) + (s & 0xffff)
    return s


def locate(frame):
    """(kind, offset of the control header, end of the message, pseudo-header bytes) of an Ethernet frame, or None."""
    if len(frame) < 14:
        return None
    et, at = struct.unpack(">H", frame[12:14])[0], 14
    while et == 0x8100 and len(frame) >= at + 4:
        et, at = struct.unpack(">H", frame[at + 2:at + 4])[0], at + 4
    if et == 0x0806:
        return "ARP", at, len(frame), b""
    if et == 0x0800 and len(frame) >= at + 20:
        ihl, total = (frame[at] & 15) * 4, struct.unpack(">H", frame[at + 2:at + 4])[0]
        frag = struct.unpack(">H", frame[at + 6:at + 8])[0] & 0x3fff
        if frame[at + 9] == 1 and not frag and total <= len(frame) - at:
            return "ICMPv4", at + ihl, at + total, b""
    if et == 0x86dd and len(frame) >= at + 40:
        plen, nh = struct.unpack(">H", frame[at + 4:at + 6])[0], frame[at + 6]
        adr, q, end = frame[at + 8:at + 40], at + 40, at + 40 + plen
        while nh in (0, 43, 60) and len(frame) >= q + 8:
            nh, q = frame[q], q + frame[q + 1] * 8 + 8
        if nh == 58 and end <= len(frame):
            return "ICMPv6", q, end, adr
    return None


def pin(kind, frame, at, end, adr):
    if kind == "ARP":
        return {}
    msg = frame[at:end]
    actual = struct.unpack(">H", msg[2:4])[0]
    zeroed = msg[:2] + b"\x00\x00" + msg[4:]
    start = 0
    if kind == "ICMPv6":
        start = ones_sum(adr) + 58 + (len(msg) & 0xffff) + (len(msg) >> 16)
    correct = ~ones_sum(zeroed, start) & 0xffff
    return dict(Valid=correct == actual, Correct=correct, Actual=actual)


def pcap_frames(path):
    raw = open(path, "rb").read()
    magic = raw[:4]
    if magic in (b"\xd4\xc3\xb2\xa1", b"\x4d\x3c\xb2\xa1"):
        e = "<"
    elif magic in (b"\xa1\xb2\xc3\xd4", b"\xa1\xb2\x3c\x4d"):
        e = ">"
    else:
        return
    if struct.unpack(e + "I", raw[20:24])[0] != 1:  # Ethernet only
        return
    q, k = 24, 0
    while q + 16 <= len(raw):
        caplen, length = struct.unpack(e + "II", raw[q + 8:q + 16])
        frame = raw[q + 16:q + 16 + caplen]
        q += 16 + caplen
        if caplen == length and len(frame) == caplen:
            yield k, frame
        k += 1


def main(ref):
    vectors = []

    def add(name, source, frame, expect):
        loc = locate(frame)
        assert loc, name
        kind, at, end, adr = loc
        p = pin(kind, frame, at, end, adr)
        assert kind == "ARP" or p["Valid"], (name, p)
        vectors.append(dict(name=name, source=source, hex=frame.hex(), kind=kind, at=at, expect=dict(expect, **p)))

    src = open(os.path.join(ref, "layers", "decode_test.go")).read()
    for var in ("testICMP", "testICMP6"):
        add(var, "layers/decode_test.go", byte_array(src, var), dict(layers=layer_list(src, var)))
    src = open(os.path.join(ref, "layers", "icmp6_test.go")).read()
    want = re.search(r"want := &ICMPv6\{(.*?)\n\t\t\}\n", src, re.S).group(1)
    add("testPacketICMPv6", "layers/icmp6_test.go", byte_array(src, "testPacketICMPv6"),
        dict(layers=layer_list(src, "testPacketICMPv6"), TypeCode=int(re.search(r"TypeCode: (\w+)", want).group(1), 16),
             Checksum=int(re.search(r"Checksum: (\w+)", want).group(1), 16), Contents=[54, 58], Payload=[58, 78]))
    src = open(os.path.join(ref, "layers", "icmp6hopbyhop_test.go")).read()
    hop = byte_array(src, "icmp6HopByHopData")
    type_at = int(re.search(r"expectedType := uint8\(icmp6HopByHopData\[(\d+)\]\)", src).group(1))
    add("icmp6HopByHopData", "layers/icmp6hopbyhop_test.go", hop,
        dict(layers=layer_list(src, "icmp6HopByHopData"), Type=hop[type_at], TypeAt=type_at))
    src = open(os.path.join(ref, "layers", "icmp6msg_test.go")).read()
    for var in ("testPacketICMPv6RouterAdvertisement", "testPacketICMPv6NeighborSolicitation"):
        add(var, "layers/icmp6msg_test.go", byte_array(src, var), dict(layers=layer_list(src, var)))
    for path in sorted(glob.glob(os.path.join(ref, "pcap", "*.pcap"))):
        for k, frame in pcap_frames(path):
            loc = locate(frame)
            if loc and (loc[0] == "ARP" or pin(*((loc[0], frame) + loc[1:]))["Valid"]):
                add("%s#%d" % (os.path.basename(path), k), "pcap/" + os.path.basename(path), frame, {})
    out = os.path.join(ROOT, "tests", "golden", "control_vectors.json")
    with open(out, "w") as f:
        json.dump(dict(vectors=vectors), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d vectors -> %s" % (len(vectors), out))


if __name__ == "__main__":
    main(sys.argv[1])
