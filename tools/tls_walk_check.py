#!/usr/bin/env python3
"""Run the TLS walk (gopacket_amd/csrc/gpk_tls_rules.h) under ASan and UBSan on
the CPU: a stand-alone program (tools/tls_walk_check.cpp, its own main, host
code only) over every case of tests/tlscases.py and the seeded corpus. Each
packet gives several messages: its TCP payload as it is, the payload from a
shifted offset (so that arbitrary bytes are walked too), and the payload with
its last 1, 7 and 40 bytes handed over as what the packet holds behind the
message (so that a ClientHello reads past the message into them, and no
further). Every buffer has its exact size: a read past the packet's end or a
write past what the size mode counted is an error. The two modes must agree
on every size, and the hello entries must account for every name byte.

    python tools/tls_walk_check.py [build directory]

It never runs on a GPU and is never loaded into Python.
"""
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def main(out_dir):
    import tlscases as C
    packets = [p for _, p in C.quirk_cases()[0]] + C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)
    corpus, n = os.path.join(out_dir, "tls_corpus.bin"), 0
    with open(corpus, "wb") as f:
        for p in packets:
            for off in (C.AT, C.AT + 5, 42):
                buf = p[off:]
                for behind in (0, 1, 7, 40):
                    if len(buf) > behind:
                        f.write(struct.pack("<II", len(buf) - behind, len(buf)) + buf)
                        n += 1
    exe = os.path.join(out_dir, "tls_walk_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "gopacket_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "tls_walk_check.cpp")])
    print("%d messages" % n)
    return subprocess.call([exe, corpus])


if __name__ == "__main__":
    if len(sys.argv) > 1:
        sys.exit(main(sys.argv[1]))
    with tempfile.TemporaryDirectory() as d:
        sys.exit(main(d))
