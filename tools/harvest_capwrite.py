#!/usr/bin/env python3
"""Harvest the byte vectors of the reference's pcap writer tests
(pcapgo/write_test.go:17-63: TestWriteHeaderNanos, TestWriteHeader,
TestWritePacket) as data into tests/golden/capwrite_vectors.json: the calls'
arguments and the bytes the tests expect. Reads the reference source as text
only; nothing of it is executed.

  python tools/harvest_capwrite.py <root of the reference's source tree>"""
import json
import os
import re
import sys

SRC = "pcapgo/write_test.go"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "capwrite_vectors.json")


def func(src, name):
    m = re.search(r"func %s\(t \*testing\.T\) \{(.*?)\n\}" % name, src, re.S)
    assert m, name
    return m.group(1)


def byte_list(body, var):
    m = re.search(r"%s := \[\]byte\{(.*?)\}" % var, body, re.S)
    assert m, var
    return bytes(int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(1)))


def num(expr):  # 0xAA*1000 and the like
    v = 1
    for f in expr.split("*"):
        v *= int(f.strip(), 0)
    return v


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    src = open(os.path.join(root, SRC)).read()
    out = {"source": SRC + ":17-63", "headers": []}
    for name, nanos in (("TestWriteHeaderNanos", True), ("TestWriteHeader", False)):
        body = func(src, name)
        a = re.search(r"WriteFileHeader\((\w+), (\w+)\)", body)
        out["headers"].append({"test": name, "nanos": nanos, "snaplen": num(a.group(1)), "linktype": num(a.group(2)),
                               "want": byte_list(body, "want").hex()})
    body = func(src, "TestWritePacket")
    ts = re.search(r"time\.Unix\(([^,]+), ([^)]+)\)", body)
    out["packet"] = {"test": "TestWritePacket", "nanos": False, "ts_sec": num(ts.group(1)), "ts_nsec": num(ts.group(2)),
                     "length": num(re.search(r"Length:\s+(\w+),", body).group(1)),
                     "capture_length": num(re.search(r"CaptureLength:\s+(\w+),", body).group(1)),
                     "data": byte_list(body, "data").hex(), "want": byte_list(body, "want").hex()}
    json.dump(out, open(OUT, "w"), indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
