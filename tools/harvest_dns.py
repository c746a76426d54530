#!/usr/bin/env python3
"""Harvest the DNS pins of the reference's tests into
tests/golden/dns_vectors.json (data only: packet bytes, and the values and
error texts the Go tests assert, read from the test files as text).

    python tools/harvest_dns.py /path/to/gopacket

  layers/dns_test.go                  every byte array a decode test uses: its link type, whether the test
                                      wants an error layer and the text it must contain, and the values the
                                      test compares (TXT, the extended response codes, URI, the OPT count and
                                      code, RRSIG, DNSKEY)
  layers/dns_dotname_test.go          the twelve messages of TestDNSDottedLabelRoundTrip, rebuilt from the
                                      labels and bytes its table names (the header and the answer frame are
                                      read from dottestHeader / dottestAnswer)
  layers/dns_svcb_regression_test.go  the two truncated SvcParams records, which must give an error

A vector: name, source, hex, link ("dns": the bytes are the message; "ethernet",
"null": a frame, the message is at `at`; "record": one resource record, wrapped
here into a message with ANCount 1), at, and expect: {"error": false} or
{"error": true, "contains": text}, plus the asserted values under the names
the tests give them.
"""
import json
import os
import re
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex_bytes(text):
    text = re.sub(r"//[^\n]*", "", text)
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{1,2})\b", text))


def byte_arrays(src):
    """name -> bytes of every `var name = []byte{...}`; `[][]byte` lists as name#k."""
    out = {}
    for m in re.finditer(r"var (\w+) = \[\]byte\{(.*?)\n\}", src, re.S):
        out[m.group(1)] = hex_bytes(m.group(2))
    for m in re.finditer(r"var (\w+) = \[\]\[\]byte\{(.*?)\n\}", src, re.S):
        for k, item in enumerate(re.findall(r"\n\t\{(.*?)\n\t\},", m.group(2), re.S)):
            out["%s#%d" % (m.group(1), k)] = hex_bytes(item)
    return out


def constants(src):
    """Go constants `Name Type = 123` of layers/dns.go, as name -> value."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^\t(\w+)\s+\w+\s+= (\d+)", src, re.M)}


def functions(src):
    """name -> body of every top-level func."""
    return {m.group(1): m.group(2) for m in re.finditer(r"^func (\w+)\(.*?\{\n(.*?)\n\}\n", src, re.S | re.M)}


def message_at(link, frame):
    if link == "ethernet":
        at = 14
    elif link == "null":
        at = 4
    else:
        return 0
    if frame[at] >> 4 == 4:
        return at + (frame[at] & 15) * 4 + 8
    return at + 40 + 8


def value(text, consts):
    text = re.sub(r"^uint\d+\((.*)\)$", r"\1", text.strip())
    if re.fullmatch(r"\d+", text):
        return int(text)
    return consts[text]


def main(ref):
    layers = os.path.join(ref, "layers")
    consts = constants(open(os.path.join(layers, "dns.go")).read())
    src = open(os.path.join(layers, "dns_test.go")).read()
    arrays, funcs = byte_arrays(src), functions(src)
    strings = dict(re.findall(r'^var (\w+) = [`"](.*?)[`"]$', src, re.M))
    numbers = {k: value(v, consts) for k, v in re.findall(r"^var (\w+) = ((?:uint16\(\d+\)|DNS\w+))$", src, re.M)}
    links = dict(LayerTypeDNS="dns", LinkTypeEthernet="ethernet", LinkTypeNull="null")
    vectors = []
    for fname, body in funcs.items():
        m = re.search(r"gopacket\.NewPacket\((\w+), (\w+), testDecodeOptions\)", body)
        rec = re.search(r"rr\.decode\((\w+), 0, nil", body)
        if fname.startswith("Test") and m and m.group(1) in arrays and "SerializeTo" not in body:
            var, link = m.group(1), links[m.group(2)]
            raw = arrays[var]
            want_err = re.search(r'errLayer == nil \{\n\t\tt\.Error\("No error layer', body) is not None
            no_err = re.search(r"ErrorLayer\(\)(; err)? != nil \{\n\t\tt\.Error\(", body) is not None
            assert want_err != no_err, fname
            e = dict(error=want_err)
            if want_err:
                e["contains"] = re.search(r'strings\.Contains\(err\.Error\(\), "(.*?)"\)', body).group(1)
            for k in ("Value", "Target"):
                if var + k in strings and var + k in body:
                    e[k] = strings[var + k]
            for k in ("ResponseCode", "Priority", "Weight"):
                if var + k in numbers and var + k in body:
                    e[k] = numbers[var + k]
            c = re.search(r"len\(optAll\) != (\d+)", body)
            if c:
                e["OPTs"] = int(c.group(1))
            c = re.search(r"OPT\[0\]\.Code != (\w+)", body)
            if c:
                e["OPTCode"] = consts[c.group(1)]
            for sec in ("questions", "answers", "additionals"):
                c = re.search(r"len\(%s\) != (\d+)" % sec, body)
                if c:
                    e[sec] = int(c.group(1))
            vectors.append(dict(name=var, source="layers/dns_test.go", hex=raw.hex(), link=link,
                                at=message_at(link, raw), expect=e))
        elif fname.startswith("TestParse") and rec:
            var = rec.group(1)
            raw = arrays[var]
            e = dict(error=False)
            for field, text in re.findall(r"if (?:rrsig|dnskey)\.(\w+) != (\S+) \{", body):
                e[field] = value(text, consts)
            c = re.search(r'string\(rrsig\.SignerName\) != "(.*?)"', body)
            if c:
                e["SignerName"] = c.group(1)
            c = re.search(r"bytes\.Equal\((?:rrsig\.Signature|dnskey\.PublicKey), %s\[len\(%s\)-(\d+):\]" % (var, var), body)
            e["Tail"] = int(c.group(1))  # Signature / PublicKey: the array's last bytes
            msg = struct.pack(">HHHHHH", 0, 0x8400, 0, 1, 0, 0) + raw
            vectors.append(dict(name=var, source="layers/dns_test.go", hex=msg.hex(), link="record", at=0, expect=e))
    for name, raw in sorted(arrays.items()):
        if "#" in name:  # testParseDNSTypeSVCB: decoded from LayerTypeDNS, a DNS layer is required
            vectors.append(dict(name=name, source="layers/dns_test.go", hex=raw.hex(), link="dns", at=0,
                                expect=dict(error=False)))

    # ---- dns_dotname_test.go: the round-trip table
    src = open(os.path.join(layers, "dns_dotname_test.go")).read()
    f = functions(src)
    head = hex_bytes(re.search(r"return \[\]byte\{(.*?)\n\t\}", f["dottestHeader"], re.S).group(1))
    assert len(head) == 8, head  # ID, flags, NSCount, ARCount; QDCount and ANCount are arguments
    frame = [hex_bytes(x) for x in re.findall(r"pkt = append\(pkt, ((?:0x\w\w(?:, )?)+)\)", f["dottestAnswer"])]
    assert [len(x) for x in frame] == [2, 4], frame  # CLASS, TTL

    def wire(*labels):
        return b"".join(bytes([len(x)]) + x.encode() for x in labels) + b"\x00"

    def header(qd, an):
        return head[:4] + struct.pack(">HH", qd, an) + head[4:]

    def answer(owner, rtype, rdata):
        return header(0, 1) + owner + struct.pack(">H", rtype) + frame[0] + frame[1] + struct.pack(">H", len(rdata)) + rdata

    body = f["TestDNSDottedLabelRoundTrip"]
    lab = lambda var: re.findall(r'"(.*?)"', re.search(r"%s := dottestWireName\((.*?)\)" % var, body).group(1))  # noqa: E731
    dotted, owner = lab("dotted"), lab("owner")
    soa = re.search(r"soa := func\(\) \[\]byte \{(.*?)\n\t\}", body, re.S).group(1)
    soa_names = [re.findall(r'"(.*?)"', x) for x in re.findall(r"dottestWireName\((.*?)\)", soa)]
    soa_tail = int(re.search(r"make\(\[\]byte, (\d+)\)", soa).group(1))
    sig = re.search(r"rrsig := func\(\) \[\]byte \{(.*?)\n\t\}", body, re.S).group(1)
    sig_fixed = int(re.search(r"make\(\[\]byte, (\d+)\)", sig).group(1))
    sig_name = re.findall(r'"(.*?)"', re.search(r"dottestWireName\((.*?)\)", sig).group(1))
    sig_tail = hex_bytes(re.search(r"return append\(rdata, (.*?)\)", sig).group(1))
    qtype = consts[re.search(r"byte\((DNSType\w+)>>8\)", body).group(1)]
    for nm, expr in re.findall(r'\{"(.*?)", (.*)\},\n', body):
        e = dict(error=False)
        if expr == "mkQuestion()":
            msg = header(1, 0) + wire(*dotted) + struct.pack(">HH", qtype, 1)
            e["Name"] = ".".join(dotted)
        else:
            m = re.match(r"dottestAnswer\((\w+), (DNSType\w+), (.*)\)$", expr)
            own, rtype, rd = m.group(1), consts[m.group(2)], m.group(3)
            e["Name"] = ".".join(dotted if own == "dotted" else owner)
            if rd == "dotted":
                rdata = wire(*dotted)
            elif rd == "soa()":
                rdata = b"".join(wire(*x) for x in soa_names) + bytes(soa_tail)
                e["RDataName"], e["RDataName2"] = (".".join(x) for x in soa_names)
            elif rd == "rrsig()":
                rdata = bytes(sig_fixed) + wire(*sig_name) + sig_tail
                e["RDataName"] = ".".join(sig_name)
            elif rd.startswith("append("):
                rdata = hex_bytes(re.search(r"\[\]byte\{(.*?)\}", rd).group(1)) + wire(*dotted)
            else:
                rdata = bytes(int(x) for x in re.search(r"\[\]byte\{(.*?)\}", rd).group(1).split(", "))
            if own != "dotted" and "RDataName" not in e:
                e["RDataName"] = ".".join(dotted)
            msg = answer(wire(*(dotted if own == "dotted" else owner)), rtype, rdata)
        vectors.append(dict(name="dotname: " + nm, source="layers/dns_dotname_test.go", hex=msg.hex(), link="dns", at=0,
                            expect=e))

    # ---- dns_svcb_regression_test.go
    src = open(os.path.join(layers, "dns_svcb_regression_test.go")).read()
    rdata = hex_bytes(re.search(r"rdata := \[\]byte\{(.*?)\}", src).group(1))
    own = re.findall(r'"(.*?)"', re.search(r"dottestWireName\((.*?)\)", src).group(1))
    for t in re.findall(r"DNSType\w+", re.search(r"range \[\]DNSType\{(.*?)\}", src).group(1)):
        vectors.append(dict(name="svcb truncated params: " + t, source="layers/dns_svcb_regression_test.go",
                            hex=answer(wire(*own), consts[t], rdata).hex(), link="dns", at=0,
                            expect=dict(error=True, contains="")))
    out = os.path.join(ROOT, "tests", "golden", "dns_vectors.json")
    with open(out, "w") as fh:
        json.dump(dict(vectors=vectors), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d vectors -> %s" % (len(vectors), out))


if __name__ == "__main__":
    main(sys.argv[1])
