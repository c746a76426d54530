#!/usr/bin/env python3
"""Build tools/svc_walk_check.cpp with AddressSanitizer + UBSan (host code only,
a stand-alone program with its own main) and run both forms of the UDP service
walk over every message of the hand-derived cases, the harvested vectors and
the seeded corpus (tests/svccases.py), each message in a heap block of exactly
its length and each entry buffer at exactly its size. The program's records
and entries are then compared, whole, with the model's (tests/svc_model.py).

    python tools/svc_walk_check.py [--keep DIR]

Nothing here is loaded into Python under a sanitizer and nothing touches a GPU.
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(out_dir):
    exe = os.path.join(out_dir, "svc_walk_check")
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tools", "svc_walk_check.cpp")]
    subprocess.run(cmd, check=True, timeout=900)
    return exe


def messages():
    """[(layer type, hdr_off, message bytes, model record dict)] of every candidate of cases, vectors and corpus."""
    import numpy as np
    import configs
    import svc_model as M
    import svccases as C
    from svcutil import GOLDEN_PACKETS, PACKETS, corpus
    from pktutil import pack
    pk = PACKETS + GOLDEN_PACKETS + corpus()
    data, offs, caps = pack(pk)
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    T = M.Tables(C.PARSER)
    raw = bytes(np.ascontiguousarray(data, np.uint8))
    out = []
    for i, p in enumerate(pk):
        cls, t = M.svc_packet(T, raw[int(offs[i]):int(offs[i]) + int(caps[i])], ref["records"][i], ref["layouts"][i], M.ALL)
        if cls >= 0:
            h = t["hdr_off"]
            out.append((t["layer_type"], h, p[h:h + t["_len"]], t))
    return out


def expected(msgs):
    import numpy as np
    from gopacket_amd import _lib
    blob = []
    for lt, h, body, t in msgs:
        rec = np.zeros(1, _lib.SVC_DTYPE)
        for name in _lib.SVC_DTYPE.names:
            if name in t:
                rec[name] = t[name]
        blob.append(rec.tobytes())
        for e in t["entries"]:
            row = np.zeros(1, _lib.SVC_ENTRY_DTYPE)
            for name, val in e.items():
                row[name] = val
            blob.append(row.tobytes())
    return b"".join(blob)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--keep", help="build and leave the files in this directory")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        os.makedirs(work, exist_ok=True)
        exe = build(work)
        msgs = messages()
        src, dst = os.path.join(work, "messages.bin"), os.path.join(work, "walk.bin")
        with open(src, "wb") as f:
            f.write(b"SVCW" + struct.pack("<I", len(msgs)))
            for lt, h, body, _ in msgs:
                f.write(struct.pack("<III", lt, h, len(body)) + body)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600, env=env)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        if r.returncode or "ERROR" in r.stderr or "runtime error" in r.stderr:
            return 1
        got, want = open(dst, "rb").read(), expected(msgs)
        if got != want:
            print("svc_walk_check: the program's %d bytes differ from the model's %d" % (len(got), len(want)))
            return 1
        print("svc_walk_check: %d messages identical to the model, no sanitizer report" % len(msgs))
    return 0


if __name__ == "__main__":
    sys.exit(main())
