#!/usr/bin/env python3
"""Harvest the TLS pins of the reference's tests into
tests/golden/tls_vectors.json (data only: packet bytes, and the values the Go
tests assert, read from the test file as text).

    python tools/harvest_tls.py /path/to/gopacket

  layers/tls_test.go   every byte array; for each decode test that uses one: whether it wants an error
                       layer, the layer list of checkLayers, and the struct literal it compares with
                       (reflect.DeepEqual), field for field. The positional literals take their field
                       names from the struct definitions of layers/tls*.go.

A vector: name, hex, link ("ethernet": a whole frame, the message is at `at`;
"tls": the bytes are the message), at, tests (the Go tests that decode it),
expect: null (no test decodes it) or {"error": bool, "layers": [names] or null,
"decoded": the struct or null}. In a decoded struct a byte slice is {"hex":
...}, nil is null, an embedded struct is a field under its type's name. The
serialization tests are not harvested: TLS.SerializeTo is not built.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hex_bytes(text):
    text = re.sub(r"//[^\n]*", "", text)
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{1,2})\b", text))


def struct_fields(src):
    """type name -> field names in order (an embedded struct under its type's name)."""
    out = {}
    for m in re.finditer(r"^type (\w+) struct \{\n(.*?)^\}", src, re.S | re.M):
        names = []
        for line in m.group(2).splitlines():
            line = re.sub(r"//.*", "", line).strip()
            if line:
                names.append(line.split()[0])
        out[m.group(1)] = names
    return out


class Literal:
    """A Go composite literal of the test file, as Python values."""

    def __init__(self, text, arrays, fields):
        self.tok = re.findall(r"0x[0-9a-fA-F]+|\d+|\w+|\[\]|[{}\[\]:,&+]", re.sub(r"//[^\n]*", "", text))
        self.i, self.arrays, self.fields = 0, arrays, fields

    def peek(self):
        return self.tok[self.i] if self.i < len(self.tok) else None

    def take(self, want=None):
        t = self.tok[self.i]
        assert want is None or t == want, (t, want, self.tok[max(0, self.i - 5):self.i + 5])
        self.i += 1
        return t

    def number(self):
        v = int(self.take(), 0)
        while self.peek() == "+":
            self.take()
            v += int(self.take(), 0)
        return v

    def value(self, elem=None):
        t = self.peek()
        if t == "&":
            self.take()
            return self.value()
        if t == "{":
            return self.body(elem)
        if t == "[]":
            self.take()
            typ = self.take()
            if typ in ("uint8", "byte"):
                self.take("{")
                vals = []
                while self.peek() != "}":
                    vals.append(self.number())
                    if self.peek() == ",":
                        self.take()
                self.take("}")
                return dict(hex=bytes(vals).hex())
            self.take("{")
            vals = []
            while self.peek() != "}":
                vals.append(self.value(typ))
                if self.peek() == ",":
                    self.take()
            self.take("}")
            return vals
        if t == "nil":
            self.take()
            return None
        if re.fullmatch(r"0x[0-9a-fA-F]+|\d+", t):
            return self.number()
        name = self.take()
        if name in self.arrays:  # a byte array, maybe sliced
            raw = self.arrays[name]
            if self.peek() == "[":
                self.take()
                lo = self.number() if self.peek() != ":" else 0
                self.take(":")
                hi = self.number() if self.peek() != "]" else len(raw)
                self.take("]")
                raw = raw[lo:hi]
            return dict(hex=raw.hex())
        assert self.peek() == "{", name
        return self.body(name)

    def body(self, typ):
        self.take("{")
        out, k = {}, 0
        while self.peek() != "}":
            if self.tok[self.i + 1] == ":" and self.tok[self.i] in self.fields[typ]:
                key = self.take()
                self.take(":")
            else:
                key = self.fields[typ][k]
            k += 1
            out[key] = self.value(key if key in self.fields else None)
            if self.peek() == ",":
                self.take()
        self.take("}")
        return out


def main(ref):
    layers = os.path.join(ref, "layers")
    fields = {"BaseLayer": ["Contents", "Payload"]}
    for f in ("tls.go", "tls_handshake.go", "tls_alert.go", "tls_cipherspec.go", "tls_appdata.go"):
        fields.update(struct_fields(open(os.path.join(layers, f)).read()))
    src = open(os.path.join(layers, "tls_test.go")).read()
    arrays = {m.group(1): hex_bytes(m.group(2)) for m in re.finditer(r"^var (\w+) = \[\]byte\{(.*?)\n\}", src, re.S | re.M)}
    decoded = {m.group(1): Literal(m.group(2), arrays, fields).value()
               for m in re.finditer(r"^var (\w+) = (&TLS\{.*?\n\})", src, re.S | re.M)}
    funcs = {m.group(1): m.group(2) for m in re.finditer(r"^func (\w+)\(.*?\{\n(.*?)\n\}\n", src, re.S | re.M)}
    expect, tests, derived = {}, {}, {}
    for fname, body in funcs.items():
        if "SerializeLayers" in body:
            continue
        m = re.search(r"gopacket\.NewPacket\((\w+)(?:\[(\d+):(\d+)\])?, (\w+), testTLSDecodeOptions\)", body)
        d = re.search(r"got\.DecodeFromBytes\((\w+), gopacket\.NilDecodeFeedback\); err != nil", body)
        if m:
            var, link = m.group(1), "ethernet" if m.group(4) == "LinkTypeEthernet" else "tls"
            name = var
            if var not in arrays:  # a copy of an array with bytes overwritten
                base = re.search(r"copy\(%s, (\w+)\)" % var, body).group(1)
                raw = bytearray(arrays[base])
                for idx, val in re.findall(r"%s\[(\d+)\] = (0x\w+)" % var, body):
                    raw[int(idx)] = int(val, 16)
                derived[var] = (bytes(raw), link)
            elif m.group(2) is not None:
                name = "%s[%s:%s]" % (var, m.group(2), m.group(3))
                derived[name] = (arrays[var][int(m.group(2)):int(m.group(3))], link)
            want_err = "ErrorLayer() == nil" in body
            lay = re.search(r"checkLayers\(p, \[\]gopacket\.LayerType\{(.*?)\}", body)
            want = re.search(r"want := (\w+)", body)
            e = dict(error=want_err, link=link,
                     layers=[x.replace("LayerType", "") for x in lay.group(1).split(", ")] if lay else None,
                     decoded=decoded[want.group(1)] if want else None)
        elif d:
            name = d.group(1)
            e = dict(error=False, link="tls", layers=None, decoded=decoded[re.search(r"want := \*(\w+)", body).group(1)])
        else:
            continue
        tests.setdefault(name, []).append(fname)
        if name in expect:
            assert expect[name]["error"] == e["error"] and expect[name]["decoded"] == e["decoded"], name
            e["layers"] = e["layers"] or expect[name]["layers"]
        expect[name] = e
    vectors = []
    for name, raw in list(arrays.items()) + [(k, v[0]) for k, v in derived.items()]:
        e = expect.get(name)
        link = e.pop("link") if e else "tls"
        at = 0
        if link == "ethernet":
            at = 14 + (raw[14] & 15) * 4
            at += (raw[at + 12] >> 4) * 4
        vectors.append(dict(name=name, source="layers/tls_test.go", hex=raw.hex(), link=link, at=at,
                            tests=sorted(tests.get(name, [])), expect=e))
    out = os.path.join(ROOT, "tests", "golden", "tls_vectors.json")
    with open(out, "w") as fh:
        json.dump(dict(vectors=vectors), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d vectors -> %s" % (len(vectors), out))


if __name__ == "__main__":
    main(sys.argv[1])
