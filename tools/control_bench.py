#!/usr/bin/env python3
"""Measure gpk_control_batch (include/gpk_control.h) on one GPU.

Input: 1 Mi-packet batches generated in HBM (gopacket_amd.synth), control
headers put in front of packets on the device (the packet becomes the
message's data), as tools/tunnel_bench.py encapsulates:
  imix_1_in_64   C4 (IMIX), every 64th packet behind Ethernet / IPv4 / ICMPv4
                 echo: the pass where control traffic is rare
  icmp4_1500     C3 (1500-byte TCP), every packet behind Ethernet / IPv4 /
                 ICMPv4 echo: pass and sum separately
  icmp6_1500     the same behind Ethernet / IPv6 / ICMPv6 echo request: the sum
                 with the pseudo-header start value
Per batch, median (min..max) over --runs timed runs after --warmup: the whole
call between two events without and with GPK_CTL_CSUM, and its kernels from the
profiler's device timeline (classify, the scan, scatter, sum16, sum64); the
sums also as GB/s over the summed bytes. Run tools/tunnel_bench.py in the same
session for the comparison: boxes differ by several percent.

  python tools/control_bench.py --out profiles/control.json
"""
import argparse
import json
import os
import re
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# this pass's instantiation of a kernel template of csrc/gpk_postpass.h, by its demangled name
OWN = r"\b%s_kernel<.*ControlPass>"


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs)) if xs else None


def kernel_times(prof):
    kern = {}
    for e in prof.events():
        if "cuda" not in str(getattr(e, "device_type", "")).lower():
            continue
        us = getattr(e, "device_time", None)
        if us is None:
            us = getattr(e, "cuda_time", 0.0)
        kern.setdefault(e.name, []).append(us / 1000.0)
    return kern


def per_run(kern, runs, *needles):
    """Device time per run of the kernels whose name matches one of `needles` (regular expressions)."""
    tot, found = [0.0] * runs, False
    for name, v in kern.items():
        if any(re.search(q, name) for q in needles):
            if len(v) % runs:
                return None
            k, found = len(v) // runs, True
            for i in range(runs):
                tot[i] += sum(v[i * k:(i + 1) * k])
    return spread(tot) if found else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from torch.profiler import ProfilerActivity, profile

    from gopacket_amd import _lib, engine, flows, synth

    n = a.packets
    prop = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               packets=n, sum_group_bytes=_lib.CTL_SUM_GROUP_BYTES,
               method="one process, %d timed runs after %d warm-up; call times between events, kernel times from the "
                      "profiler's device timeline; medians with min..max" % (a.runs, a.warmup), rows=[])
    ctx = engine.Context(0)
    kinds = [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP,
             _lib.DEC_PAYLOAD]
    parser = engine.ParserConfig(17, kinds)
    ctd = flows.ControlDecoder(n)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")

    def encapsulate(d, o, c, header, len_at, every=1):
        """header (bytes) in front of every `every`-th packet; len_at: (byte offset, constant) pairs
        of big-endian 16-bit length fields = constant + the packet's length."""
        m = o.numel()
        hl = len(header)
        h = torch.tensor(list(header), dtype=torch.uint8, device="cuda").repeat(m, 1)
        for at, k in len_at:
            v = c + k
            h[:, at] = (v >> 8).to(torch.uint8)
            h[:, at + 1] = (v & 255).to(torch.uint8)
        ctl = (torch.arange(m, device="cuda") % every) == 0
        cat = torch.cat([h.flatten(), d])
        po = torch.stack([torch.arange(m, device="cuda", dtype=torch.int64) * hl, o + m * hl], 1).flatten()
        pc = torch.stack([torch.where(ctl, hl, 0).int(), c], 1).flatten()
        od, oo, oc = flows.pack_batch(cat, po, pc, torch.arange(2 * m, device="cuda", dtype=torch.int32))
        pad = torch.zeros((od.numel() + 15) // 16 * 16 + 32, dtype=torch.uint8, device="cuda")
        pad[:od.numel()] = od
        return pad, oo[0::2].contiguous(), (oc[0::2] + oc[1::2]).contiguous()

    mac = bytes(range(1, 13))
    ip4 = struct.pack(">BBHHHBBH", 0x45, 0, 0, 1, 0, 64, 1, 0) + bytes([10, 0, 0, 1, 10, 0, 0, 2])
    ip6 = struct.pack(">IHBB", 6 << 28, 0, 58, 64) + bytes(15) + b"\x01" + bytes(15) + b"\x02"
    icmp4_hdr = mac + b"\x08\x00" + ip4 + struct.pack(">BBHHH", 8, 0, 0x1234, 7, 1)
    icmp6_hdr = mac + b"\x86\xdd" + ip6 + struct.pack(">BBHHH", 128, 0, 0x1234, 7, 1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    rows = [("imix_1_in_64", synth.C4_IMIX, icmp4_hdr, [(16, 28)], 64, 8),
            ("icmp4_1500", synth.C3_TCP1500, icmp4_hdr, [(16, 28)], 1, 8),
            ("icmp6_1500", synth.C3_TCP1500, icmp6_hdr, [(18, 8)], 1, 8)]
    for name, cfg, header, len_at, every, msg_hdr in rows:
        d0, o0, c0 = synth.device_batch(cfg, 0, n)
        d, o, c = encapsulate(d0, o0, c0, header, len_at, every)
        del d0
        ctx.decode_device(parser, d, o, c, rec, err, fl, lay)
        out = ctd.decode(ctx, d, o, c, rec, lay, parser)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().tolist()
        sel = (torch.arange(n, device="cuda") % every) == 0
        summed = int((c0[sel].to(torch.int64) + msg_hdr).sum().item())

        def plain():
            ctd.decode(ctx, d, o, c, rec, lay, parser, checksum=False, out=out)

        def sums():
            ctd.decode(ctx, d, o, c, rec, lay, parser, checksum=True, out=out)

        calls = dict(pass_ms=plain, pass_with_sums_ms=sums)
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        ev = {k: [] for k in calls}
        for _ in range(a.runs):
            for k, f in calls.items():
                ev[k].append(timed(f))
            torch.cuda.synchronize()
        t = {k: [x.elapsed_time(y) for x, y in v] for k, v in ev.items()}
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.runs):
                sums()
                torch.cuda.synchronize()
        kern = kernel_times(prof)
        s16 = [x for k, v in kern.items() if re.search(OWN % "sum16", k) for x in v]
        s64 = [x for k, v in kern.items() if re.search(OWN % "sum64", k) for x in v]
        both = [x + y for x, y in zip(s16, s64)] if len(s16) == len(s64) else []
        row = dict(batch=name, source=synth.NAMES[cfg], control_one_in=every, packets=n, candidates=counts[0],
                   class_counts=counts[1:5], sums_made=counts[5], batch_bytes=int(c.sum(dtype=torch.int64).item()),
                   summed_bytes=summed, pass_ms=spread(t["pass_ms"]),
                   pass_Mpps=spread([n / (x * 1e3) for x in t["pass_ms"]]),
                   pass_with_sums_ms=spread(t["pass_with_sums_ms"]),
                   kernels_ms=dict(classify=per_run(kern, a.runs, OWN % "classify"),
                                   scatter=per_run(kern, a.runs, OWN % "scatter"),
                                   scan=per_run(kern, a.runs, "scan", "Scan", r"\bfinish_kernel<%d>" % _lib.CTL_NCLASS),
                                   sum16=spread(s16), sum64=spread(s64), sum=spread(both)),
                   sum_GBps=spread([summed / (x * 1e6) for x in both]))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del d, o, c, out
    ctd.close()
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
