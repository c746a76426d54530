#!/usr/bin/env python3
"""Harvest the DHCPv4, DHCPv6 and NTP pins of the reference's tests into
tests/golden/svc_vectors.json (data only: packet bytes and the values the Go
tests assert, read from the test files as text).

    python tools/harvest_svc.py /path/to/gopacket

  layers/ntp_test.go     the three Ethernet frames of TestNTPOne/Two/Three with the NTP struct each must
                         decode to, and checkNTP's checkLayers list
  layers/dhcp_test.go    the three messages TestDHCPv4Encode* build, serialize and decode again (testDHCPEqual
                         asserts every field and every option's Type and Data), and the six buffers of
                         TestDHCPv4DecodeOption with the error each must give
  layers/dhcpv6_test.go  the two messages of TestDHCPv6EncodeRequest / Reply (testDHCPv6Equal)

The DHCP tests hold no frames: they fill a struct, serialize it and compare
the decoded struct with it. This tool reads the struct literals and lays the
message out itself (RFC 2131 / RFC 8415 wire format, tests/svccases.py's
builders) behind Ethernet / IP / UDP, so a vector is, as for NTP: name, source,
hex (an Ethernet frame) and expect: "layers" and "fields" (Go field name ->
value; byte strings as hex; "Options" as [code, length, data hex]). An option
vector is: name, source, option_hex and expect "error" (Go's text, or "").
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REG = json.load(open(os.path.join(ROOT, "gopacket_amd", "registry_gen.json")))
LT = {}
for _k, _v in REG["layer_type_names"].items():
    LT.setdefault(_v.replace(" ", ""), int(_k))


def functions(src):
    """{name: body} of the file's top-level functions."""
    return {m.group(1): m.group(2) for m in re.finditer(r"^func (\w+)\(.*?\{\n(.*?)^\}", src, re.S | re.M)}


def byte_list(text, names):
    """The bytes of a Go []byte{...} body: numbers, 'c' characters and byte(NAME) of our own tables."""
    out = []
    for tok in (t.strip() for t in re.sub(r"//[^\n]*", "", text).split(",")):
        if not tok:
            continue
        m = re.fullmatch(r"byte\((\w+)\)", tok)
        if m:
            out.append(int(names[m.group(1)]))
        elif tok.startswith("'"):
            out.append(ord(tok[1]))
        else:
            out.append(int(tok, 0))
    return bytes(out)


def ntp_vectors(src, add):
    layers = [LT[n] for n in re.findall(r"LayerType(\w+)", re.search(r"checkLayers\(p, \[\]gopacket\.LayerType\{(.*?)\}", src, re.S).group(1))]
    for name, body in functions(src).items():
        m = re.search(r"var testPacketNTP = \[\]byte\{(.*?)\n\t\}", body, re.S)
        if not m:
            continue
        frame = byte_list(m.group(1), {})
        want = body[body.index("pExpectedNTP := &NTP{"):body.index("checkNTP(")]
        want = re.sub(r"BaseLayer: BaseLayer\{.*?\n\t\t\},", "", want, flags=re.S)
        fields = {k: int(v, 0) for k, v in re.findall(r"(\w+):\s+(-?(?:0x[0-9a-fA-F]+|\d+)),", want)}
        ext = re.search(r"ExtensionBytes:\s+\[\]byte\{(.*?)\}", want, re.S)
        fields["ExtensionBytes"] = byte_list(ext.group(1), {}).hex()
        add(name, "ntp_test.go", frame, layers=layers, fields=fields)


def dhcp4_vectors(src, add, add_option):
    import svccases as C
    from gopacket_amd import layers as L
    names = {k: v for k, v in vars(L).items() if k.startswith(("DHCPOpt", "DHCPMsgType"))}
    for name, body in functions(src).items():
        if "dhcp := &DHCPv4{" not in body:
            continue
        lit = body[body.index("dhcp := &DHCPv4{"):body.index("buf := gopacket.NewSerializeBuffer()")]
        op = {"DHCPOpRequest": 1, "DHCPOpReply": 2}[re.search(r"Operation: (\w+)", lit).group(1)]
        assert re.search(r"HardwareType: (\w+)", lit).group(1) == "LinkTypeEthernet"
        xid = int(re.search(r"Xid: (\w+)", lit).group(1), 0)
        ips = {k: byte_list(v, {}) for k, v in re.findall(r"(\w+IP): net\.IP\{([^}]*)\}", lit)}
        hw = byte_list(re.search(r"ClientHWAddr: net\.HardwareAddr\{([^}]*)\}", lit).group(1), {})
        opts = []
        for typ, nil, data in re.findall(r"NewDHCPOption\((\w+),\s*(?:(nil)|\[\]byte\{(.*?)\})\)\)", lit, re.S):
            opts.append((int(names[typ]), b"" if nil else byte_list(data, names)))
        wire = b"".join(C.PAD if t == 0 else C.opt4(t, d) for t, d in opts) + C.END
        msg = C.dhcp4(wire, op=op, htype=1, hlen=len(hw), xid=xid, flags=0, ciaddr=ips["ClientIP"], yiaddr=ips["YourClientIP"],
                      siaddr=ips["NextServerIP"], giaddr=ips["RelayAgentIP"], chaddr=hw)
        frame = C.over4(msg, 68, 67) if op == 1 else C.over4(msg, 67, 68)
        add(name, "dhcp_test.go", frame, layers=[LT["Ethernet"], LT["IPv4"], LT["UDP"], LT["DHCPv4"]],
            fields=dict(Operation=op, HardwareType=1, HardwareLen=len(hw), RelayHops=0, Xid=xid, Secs=0, Flags=0,
                        ClientIP=ips["ClientIP"].hex(), YourClientIP=ips["YourClientIP"].hex(),
                        NextServerIP=ips["NextServerIP"].hex(), RelayAgentIP=ips["RelayAgentIP"].hex(),
                        ClientHWAddr=hw.hex(), ServerName=bytes(64).hex(), File=bytes(128).hex(),
                        Options=[[t, len(d), d.hex()] for t, d in opts]))
    table = functions(src)["TestDHCPv4DecodeOption"]
    errors = {"nil": "", "DecOptionNotEnoughData": "Not enough data to decode", "DecOptionMalformed": "Option is malformed"}
    for msg, buf, err in re.findall(r'msg: "([^"]*)",\s*buf: (.*?),\s*err: (\w+),', table, re.S):
        if buf.startswith("bytes.Join"):
            head = byte_list(re.search(r"\{(\d+, \d+)\}", buf).group(1), {})
            rep = re.search(r"bytes\.Repeat\(\[\]byte\{(\d+)\}, (\d+)\)", buf)
            raw = head + bytes([int(rep.group(1))]) * int(rep.group(2))
        else:
            raw = byte_list(re.fullmatch(r"\[\]byte\{(.*)\}", buf.strip(), re.S).group(1), {})
        add_option(msg, "dhcp_test.go", raw, errors[err])


def dhcp6_vectors(src, add):
    import svccases as C
    from gopacket_amd import layers as L
    for name, body in functions(src).items():
        if "dhcpv6 := &DHCPv6{" not in body:
            continue
        head = re.search(r"&DHCPv6\{MsgType: (\w+), HopCount: (\d+), TransactionID: \[\]byte\{([^}]*)\}\}", body)
        typ, txid = int(getattr(L, head.group(1))), byte_list(head.group(3), {})
        opts = []
        for var, code in re.findall(r"NewDHCPv6Option\((\w+), (\w+)\.Encode\(\)\)", body):
            d = re.search(r"%s := &DHCPv6DUID\{Type: (\w+), HardwareType: \[\]byte\{([^}]*)\}, Time: \[\]byte\{([^}]*)\}, "
                          r"LinkLayerAddress: \[\]byte\{([^}]*)\}\}" % code, body)
            assert d.group(1) == "DHCPv6DUIDTypeLLT"  # RFC 8415 11.2: type 1, hardware type, time, link-layer address
            duid = b"\x00\x01" + byte_list(d.group(2), {}) + byte_list(d.group(3), {}) + byte_list(d.group(4), {})
            opts.append((int(getattr(L, var)), duid))
        msg = C.dhcp6(b"".join(C.opt6(c, d) for c, d in opts), typ, int.from_bytes(txid, "big"))
        frame = C.over6(msg, 546, 547) if typ != 7 else C.over6(msg, 547, 546)
        add(name, "dhcpv6_test.go", frame, layers=[LT["Ethernet"], LT["IPv6"], LT["UDP"], LT["DHCPv6"]],
            fields=dict(MsgType=typ, HopCount=int(head.group(2)), LinkAddr="", PeerAddr="", TransactionID=txid.hex(),
                        Options=[[c, len(d), d.hex()] for c, d in opts]))


def main(ref):
    vectors, options = [], []

    def read(name):
        return open(os.path.join(ref, "layers", name)).read()

    def add(name, source, frame, **expect):
        vectors.append(dict(name=name, source="layers/" + source, hex=frame.hex(), expect=expect))

    def add_option(name, source, raw, error):
        options.append(dict(name=name, source="layers/" + source, option_hex=raw.hex(), expect=dict(error=error)))

    ntp_vectors(read("ntp_test.go"), add)
    dhcp4_vectors(read("dhcp_test.go"), add, add_option)
    dhcp6_vectors(read("dhcpv6_test.go"), add)
    out = os.path.join(ROOT, "tests", "golden", "svc_vectors.json")
    with open(out, "w") as f:
        json.dump(dict(vectors=vectors, options=options), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d vectors, %d option vectors -> %s" % (len(vectors), len(options), out))


if __name__ == "__main__":
    main(sys.argv[1])
