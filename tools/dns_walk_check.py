#!/usr/bin/env python3
"""Run the DNS walk (gopacket_amd/csrc/gpk_dns_rules.h) under ASan and UBSan on
the CPU: a stand-alone program (tools/dns_walk_check.cpp, its own main, host
code only) over every case of tests/dnscases.py and the seeded corpus, each
packet's bytes taken as a message from its UDP payload, its TCP payload and a
shifted offset, so that arbitrary bytes are walked too. Every buffer has its
exact size: a read past a message or a write past what the size mode counted
is an error. The two modes must agree on every size.

    python tools/dns_walk_check.py [build directory]
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
    import dnscases as C
    packets = [p for _, p in C.quirk_cases()[0]] + C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)
    corpus, n = os.path.join(out_dir, "dns_corpus.bin"), 0
    with open(corpus, "wb") as f:
        for p in packets:
            for off in (42, 54, 56):
                if p[off:]:
                    f.write(struct.pack("<I", len(p) - off) + p[off:])
                    n += 1
    exe = os.path.join(out_dir, "dns_walk_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "gopacket_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "dns_walk_check.cpp")])
    print("%d messages" % n)
    return subprocess.call([exe, corpus])


if __name__ == "__main__":
    if len(sys.argv) > 1:
        sys.exit(main(sys.argv[1]))
    with tempfile.TemporaryDirectory() as d:
        sys.exit(main(d))
