#!/usr/bin/env python3
"""Measure gpk_ndp_batch (include/gpk_ndp.h) on one GPU, beside
gpk_control_batch on the same batches in the same session: the NDP pass is the
control pass's shape plus a second scan and an emit kernel, so that is its
yardstick.

Input: 1 Mi-packet batches in HBM. The first three repeat one frame (Ethernet /
IPv6 / ICMPv6 / message); the last is IMIX (gopacket_amd.synth C4) with every
64th packet replaced by such a frame:
  ns_1_option        Neighbor Solicitation with a Source Link-Layer Address option
  ra_4_options       Router Advertisement with SLLA, MTU, Prefix Information, RDNSS
  mld2_8_records     MLDv2 report of eight records without sources
  imix_1_in_64       IMIX, every 64th packet the Neighbor Solicitation
Per batch, median (min..max) over --runs timed runs after --warmup: the whole
gpk_ndp_batch call between two events with the capacity the batch needs, the
sizing call with capacity 0, the control pass with and without its sums, and
the NDP call's kernels from the profiler's device timeline (classify, the first
scan with finish, scatter, the second scan, emit).

  python tools/ndp_bench.py --out profiles/ndp.json
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

OWN = r"\b%s_kernel<.*NdpPass>"  # this pass's instantiation of a kernel template of csrc/gpk_postpass.h


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


def frames():
    """The three frames, checksums not set (the NDP pass does not look at them)."""
    mac = bytes(range(1, 13)) + b"\x86\xdd"

    def frame(icmp_type, body):
        msg = struct.pack(">BBH", icmp_type, 0, 0) + body
        ip6 = struct.pack(">IHBB", 6 << 28, len(msg), 58, 255) + bytes.fromhex("fe80" + "00" * 13 + "01") + \
            bytes.fromhex("ff02" + "00" * 13 + "01")
        return mac + ip6 + msg

    def opt(typ, data):
        return bytes([typ, (len(data) + 2) // 8]) + data
    lla = opt(1, bytes.fromhex("000c290e4c67"))
    target = bytes.fromhex("fe80000000000000020c29fffe0e4c67")
    ns = frame(135, bytes(4) + target + lla)
    ra = frame(134, struct.pack(">BBHII", 64, 0x40, 1800, 0, 0) + lla + opt(5, bytes(2) + struct.pack(">I", 1500)) +
               opt(3, struct.pack(">BBIII", 64, 0xc0, 2592000, 604800, 0) + bytes.fromhex("20010db8" + "00" * 12)) +
               opt(25, bytes(2) + struct.pack(">I", 600) + bytes.fromhex("20010db8" + "00" * 11 + "53")))
    rec = b"".join(struct.pack(">BBH", 2, 0, 0) + bytes.fromhex("ff02" + "00" * 12) + bytes([1, k]) for k in range(8))
    mld = frame(143, struct.pack(">HH", 0, 8) + rec)
    return dict(ns_1_option=ns, ra_4_options=ra, mld2_8_records=mld)


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
               packets=n,
               method="one process, %d timed runs after %d warm-up; call times between events, kernel times from the "
                      "profiler's device timeline; medians with min..max; the control pass on the same batch in the "
                      "same loop" % (a.runs, a.warmup), rows=[])
    ctx = engine.Context(0)
    kinds = [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP,
             _lib.DEC_PAYLOAD]
    parser = engine.ParserConfig(17, kinds)
    ndd, ctd = flows.NDPDecoder(n), flows.ControlDecoder(n)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    fr = frames()

    def repeated(frame, count):
        stride = (len(frame) + 15) // 16 * 16
        row = torch.zeros(stride, dtype=torch.uint8)
        row[:len(frame)] = torch.tensor(list(frame), dtype=torch.uint8)
        d = torch.cat([row.cuda().repeat(count), torch.zeros(32, dtype=torch.uint8, device="cuda")])
        o = torch.arange(count, device="cuda", dtype=torch.int64) * stride
        c = torch.full((count,), len(frame), dtype=torch.int32, device="cuda")
        return d, o, c

    def imix(frame, every):
        d0, o0, c0 = synth.device_batch(synth.C4_IMIX, 0, n)
        base = (d0.numel() + 15) // 16 * 16
        fd, fo, fc = repeated(frame, (n + every - 1) // every)
        d = torch.cat([d0, torch.zeros(base - d0.numel(), dtype=torch.uint8, device="cuda"), fd])
        idx = torch.arange(n, device="cuda")
        sel = idx % every == 0
        o = torch.where(sel, fo[idx // every] + base, o0)
        c = torch.where(sel, fc[idx // every], c0)
        return d, o.contiguous(), c.contiguous()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    batches = [(name, lambda f=f: repeated(f, n), 1) for name, f in fr.items()]
    batches.append(("imix_1_in_64", lambda: imix(fr["ns_1_option"], 64), 64))
    for name, make, every in batches:
        d, o, c = make()
        ctx.decode_device(parser, d, o, c, rec, err, fl, lay)
        sized = ndd.decode(ctx, d, o, c, rec, lay, parser, 0)
        torch.cuda.synchronize()
        need = flows.NDPDecoder.needed(sized["counts"].cpu().numpy().view("u4"))
        out = ndd.decode(ctx, d, o, c, rec, lay, parser, need)
        cout = ctd.decode(ctx, d, o, c, rec, lay, parser)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().numpy().view("u4").tolist()
        assert not counts[3] and counts[2] == 0 and counts[0] == (n + every - 1) // every, counts

        calls = dict(ndp_ms=lambda: ndd.decode(ctx, d, o, c, rec, lay, parser, need, out=out),
                     ndp_sizing_ms=lambda: ndd.decode(ctx, d, o, c, rec, lay, parser, 0, out=sized),
                     control_ms=lambda: ctd.decode(ctx, d, o, c, rec, lay, parser, checksum=False, out=cout),
                     control_with_sums_ms=lambda: ctd.decode(ctx, d, o, c, rec, lay, parser, checksum=True, out=cout))
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        ev = {k: [] for k in calls}
        for _ in range(a.runs):
            for k, f in calls.items():
                ev[k].append(timed(f))
            torch.cuda.synchronize()
        t = {k: spread([x.elapsed_time(y) for x, y in v]) for k, v in ev.items()}
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.runs):
                calls["ndp_ms"]()
                torch.cuda.synchronize()
        kern = kernel_times(prof)
        scans = per_run(kern, a.runs, "scan", "Scan", r"\bfinish_kernel<%d>" % _lib.NDP_NCLASS)
        row = dict(batch=name, ndp_one_in=every, packets=n, candidates=counts[0], entries=need,
                   batch_bytes=int(c.sum(dtype=torch.int64).item()), **t,
                   ndp_messages_per_s=counts[0] / (t["ndp_ms"]["median"] * 1e-3),
                   kernels_ms=dict(classify=per_run(kern, a.runs, OWN % "classify"),
                                   scatter=per_run(kern, a.runs, OWN % "scatter"), scans_and_finish=scans,
                                   emit=per_run(kern, a.runs, r"\bemit_kernel")))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del d, o, c, out, sized, cout
    ndd.close()
    ctd.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
