#!/usr/bin/env python3
"""Measure gpk_tls_batch (include/gpk_tls.h) on one GPU.

Batches of --packets packets (default 1 Mi):
  appdata_1      every packet a 1448-byte TCP segment of one Application Data
                 record: the common case, every packet a candidate
  appdata_2      the same segment as two records of 719 bytes
  client_hello   every packet the ClientHello frame of the reference's tests
                 (tests/golden/tls_vectors.json), with its server name
  imix_1_in_4    C4 (IMIX) generated in HBM (gopacket_amd.synth), every fourth
                 packet behind Ethernet / IPv4 / TCP port 443 and the header of
                 an Application Data record whose body is the packet
and one batch of --adversarial (default 1 Ki) packets:
  empty_300      300 empty Application Data records in 1500 bytes: the most
                 records a 1500-byte message holds
Per batch, median (min..max) over --runs timed runs after --warmup: the whole
call between two events, with capacities that hold everything. The kernels'
own times come from a profiler run of their own, one per batch:

  rocprofv3 --kernel-trace --stats -d DIR/BATCH -o tls -- python tools/tls_bench.py --only BATCH
  python tools/tls_bench.py --out profiles/tls.json --stats DIR

--stats reads each DIR/BATCH/**/*kernel_stats.csv and adds, per kernel of the
pass, the calls and the average duration the profiler saw (warm-up and sizing
calls included: they run the same kernels on the same batch).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAC = bytes(range(1, 13))
BATCHES = ("appdata_1", "appdata_2", "client_hello", "imix_1_in_4", "empty_300")
KERNELS = (("classify", "classify_kernel"), ("scatter", "scatter_kernel"), ("emit", "emit_kernel"),
           ("finish", "finish_kernel"), ("scan", "scan"))


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs)) if xs else None


def rec(ct, body=b"", ver=0x0303):
    return struct.pack(">BHH", ct, ver, len(body)) + body


def frame(msg, dport=443):
    tcp = struct.pack(">HHIIBBHHH", 40000, dport, 1, 2, 0x50, 0x18, 1000, 0, 0) + msg
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(tcp), 1, 0, 64, 6, 0) + bytes([10, 0, 0, 1, 10, 0, 0, 2]) + tcp
    return MAC + b"\x08\x00" + ip


def kernel_stats(path):
    """{kernel of the pass: {calls, average_us}} from the profiler's kernel statistics of one batch."""
    out = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name") or row.get("KernelName") or ""
            if "pack_" in name or "decode_kernel" in name:  # the batch's own making
                continue
            for key, needle in KERNELS:
                if needle in name.lower():
                    calls = int(row["Calls"])
                    total = float(row["TotalDurationNs"])
                    cur = out.setdefault(key, dict(calls=0, total_us=0.0))
                    cur["calls"] += calls
                    cur["total_us"] += total / 1000.0
                    break
    for v in out.values():
        v["average_us"] = v["total_us"] / v["calls"] if v["calls"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--adversarial", type=int, default=1 << 10)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=BATCHES, help="one batch (for a profiler run)")
    ap.add_argument("--stats", help="directory of the profiler runs, one subdirectory per batch")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    from gopacket_amd import _lib, engine, flows, synth

    n = a.packets
    prop = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               shape="one lane per message in classify, scatter and emit",
               method="one process, %d timed runs after %d warm-up; call times between events; medians with min..max; "
                      "kernel times from rocprofv3 --kernel-trace --stats, one run per batch" % (a.runs, a.warmup),
               rows=[])
    ctx = engine.Context(0)
    kinds = [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP,
             _lib.DEC_PAYLOAD]
    parser = engine.ParserConfig(17, kinds)

    def encapsulate(d, o, c, header, len_at, every):
        """tools/control_bench.py's: header in front of every `every`-th packet, its length fields set."""
        m = o.numel()
        hl = len(header)
        h = torch.tensor(list(header), dtype=torch.uint8, device="cuda").repeat(m, 1)
        for at, k in len_at:
            v = c + k
            h[:, at] = (v >> 8).to(torch.uint8)
            h[:, at + 1] = (v & 255).to(torch.uint8)
        sel = (torch.arange(m, device="cuda") % every) == 0
        cat = torch.cat([h.flatten(), d])
        po = torch.stack([torch.arange(m, device="cuda", dtype=torch.int64) * hl, o + m * hl], 1).flatten()
        pc = torch.stack([torch.where(sel, hl, 0).int(), c], 1).flatten()
        od, oo, oc = flows.pack_batch(cat, po, pc, torch.arange(2 * m, device="cuda", dtype=torch.int32))
        pad = torch.zeros((od.numel() + 15) // 16 * 16 + 32, dtype=torch.uint8, device="cuda")
        pad[:od.numel()] = od
        return pad, oo[0::2].contiguous(), (oc[0::2] + oc[1::2]).contiguous()

    def tiled(pkt, count):
        stride = (len(pkt) + 15) // 16 * 16
        row = np.zeros(stride, np.uint8)
        row[:len(pkt)] = np.frombuffer(pkt, np.uint8)
        d = torch.from_numpy(np.concatenate([np.tile(row, count), np.zeros(32, np.uint8)])).cuda()
        o = torch.arange(count, dtype=torch.int64, device="cuda") * stride
        c = torch.full((count,), len(pkt), dtype=torch.int32, device="cuda")
        return d, o, c

    def measure(label, d, o, c, extra):
        m = o.numel()
        rec_ = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
        err = torch.zeros(2 * m, dtype=torch.int32, device="cuda")
        fl = torch.zeros(3 * m, dtype=torch.int64, device="cuda")
        lay = torch.zeros(m * 64, dtype=torch.uint8, device="cuda")
        ctx.decode_device(parser, d, o, c, rec_, err, fl, lay)
        tld = flows.TLSDecoder(m)
        out = tld.decode_all(ctx, d, o, c, rec_, lay, parser)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().numpy().view(np.uint32)
        need = flows.TLSDecoder.needed(counts)

        def call():
            tld.decode(ctx, d, o, c, rec_, lay, parser, *need, out=out)

        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        msgs = int(counts[0])
        written = (4 * m + 4 * msgs + _lib.TLS_DTYPE.itemsize * msgs + _lib.TLS_REC_DTYPE.itemsize * need[0] +
                   _lib.TLS_HELLO_DTYPE.itemsize * need[1] + need[2])
        row = dict(batch=label, packets=m, candidates=msgs, ok=int(counts[1]), failed=int(counts[2]), records=need[0],
                   hellos=need[1], sni_bytes=need[2], batch_bytes=int(c.sum(dtype=torch.int64).item()),
                   bytes_written=written, bytes_written_per_packet=written / m, pass_ms=spread(t),
                   messages_per_s=spread([msgs / (x * 1e-3) for x in t]) if msgs else None,
                   ns_per_packet=statistics.median(t) * 1e6 / m, **extra)
        if a.stats:
            row["kernels"] = kernel_stats(os.path.join(a.stats, label)) or None
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        tld.close()

    def want(label):
        return a.only in (None, label)

    if want("appdata_1"):
        measure("appdata_1", *tiled(frame(rec(23, bytes(1443))), n), dict(message_bytes=1448, records_per_message=1))
    if want("appdata_2"):
        measure("appdata_2", *tiled(frame(rec(23, bytes(719)) * 2), n), dict(message_bytes=1448, records_per_message=2))
    if want("client_hello"):
        vec = json.load(open(os.path.join(ROOT, "tests", "golden", "tls_vectors.json")))["vectors"]
        hello = bytes.fromhex(next(v["hex"] for v in vec if v["name"] == "testClientHello"))
        measure("client_hello", *tiled(hello, n), dict(message_bytes=len(hello) - 54, server_name="www.google.com"))
    if want("imix_1_in_4"):
        hdr = frame(b"\x17\x03\x03\x00\x00")
        d0, o0, c0 = synth.device_batch(synth.C4_IMIX, 0, n)
        d, o, c = encapsulate(d0, o0, c0, hdr, [(16, len(hdr) - 14), (len(hdr) - 2, 0)], 4)
        del d0
        measure("imix_1_in_4", d, o, c, dict(source=synth.NAMES[synth.C4_IMIX], tls_one_in=4))
        del d, o, c
    if want("empty_300"):
        measure("empty_300", *tiled(frame(rec(23) * 300), a.adversarial), dict(message_bytes=1500, records_per_message=300))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
