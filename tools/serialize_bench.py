#!/usr/bin/env python3
"""Measure gpk_serialize_batch (include/gpk_serialize.h) on one GPU against the
capture writer's framing kernel, which is the same move without the sum and
without header rebuilding.

Input: 1 Mi-packet batches of the C2 (64-byte UDP), C3 (1500-byte TCP) and C4
(IMIX) shapes generated in HBM (gopacket_amd.synth) and decoded on the device
with layouts and fields. Per batch, for each of the four option sets and both
group sizes of the write kernel, median (min..max) over --runs timed runs after
--warmup, the kernels alternating inside every run so drift hits all alike:
  move      ser_move_kernel (the tails, with the sum when ComputeChecksums)
  head      ser_head_kernel (the headers, gaps and pads; one lane per packet, the
            same at both group sizes: all its launches pooled)
  write     move + the median head: kernel times from the profiler's device
            timeline, GB/s moved (bytes read + bytes written) and Mpkts/s
  frame     gpk_capwrite_batch's frame_kernel on the same packets, pcap format,
            same group size: the yardstick
  ratio     move time / frame time and write time / frame time
  e2e       the whole gpk_serialize_batch call (size kernel, scan, counts,
            write) between two events
The crossover table runs the move kernel at both group sizes over uniform
packets: the C3 batch with its capture lengths cut and decoded again
("decoded"), and packets without any layer, which are one verbatim tail, up to
9000 bytes ("raw"). kGroup16MaxMean of gpk_serialize.hip is read off it.

  python tools/serialize_bench.py --out profiles/serialize.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


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


def pick(kern, *pieces):
    out = []
    for name, xs in kern.items():
        if all(any(q in name for q in p) for p in pieces):
            out += xs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=1792,
                    help="kGroup16MaxMean of gpk_serialize.hip, recorded next to the table it came from")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from torch.profiler import ProfilerActivity, profile

    from gopacket_amd import _lib, engine, synth
    from gopacket_amd.flows import Serializer

    L = _lib.lib()
    st = torch.cuda.current_stream()
    prop = torch.cuda.get_device_properties(0)
    n = a.packets
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               packets=n,
               method="one process, kernels alternating inside every run, %d timed runs after %d warm-up; kernel times "
                      "from the profiler's device timeline, e2e between events; medians with min..max; GB/s counts the "
                      "bytes read plus the bytes written" % (a.runs, a.warmup), rows=[], crossover=[])
    ctx = engine.Context(0)
    parser = engine.ParserConfig(17, [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6,
                                      _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP, _lib.DEC_PAYLOAD])
    ser = Serializer(n, device=0)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    f = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
    h = ctypes.c_void_p()
    _lib.check(L.gpk_capwriter_create(ctypes.byref(h), _lib.CAPW_PCAP_NANO, 0, n))
    ci = torch.zeros((n, 6), dtype=torch.int32, device="cuda")  # gpk_capture_info as int32 words
    ci[:, 0] = 1600000000
    ci[:, 5] = -1
    boff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    stt = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")

    def measure(d, o, c, m, label, optsets, decoded=True):
        """write vs frame at both groups for the option sets; returns rows"""
        if decoded:
            ctx.decode_device_fields(parser, d, o, c, rec, err, fl, f, layouts=lay, stream=st)
        else:  # no layer: the whole packet is one verbatim tail
            lay.fill_(0xFF)
            f.zero_()
        ci[:, 3] = c
        payload = int(c[:m].sum(dtype=torch.int64).item())
        cap = payload + 128 * m
        out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
        b = _lib.Batch(d.data_ptr(), o.data_ptr(), c.data_ptr(), m, d.numel())

        def write(fix, csum, group):
            return ser.serialize(d, o[:m], c[:m], lay, f, None, fix, csum, out=out, out_cap=cap, group=group, stream=st)

        def frame(group):
            op = _lib.CapwriteOpts(0, 0, group)
            _lib.check(L.gpk_capwrite_batch(h, ctypes.byref(b), None, m, ci.data_ptr(), None, None, ctypes.byref(op),
                                            out.data_ptr(), cap, boff.data_ptr(), stt.data_ptr(), cnt.data_ptr(),
                                            st.cuda_stream))

        rows = []
        for fix, csum in optsets:
            r = write(fix, csum, 0)
            torch.cuda.synchronize()
            counts = r["counts"].cpu().tolist()
            assert counts[3] == 0, counts
            written = counts[1]
            for _ in range(a.warmup):
                for g in (16, 64):
                    write(fix, csum, g)
                    frame(g)
            torch.cuda.synchronize()
            e2e = {16: [], 64: []}
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(a.runs):
                    for g in (16, 64):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        write(fix, csum, g)
                        e1.record()
                        frame(g)
                        torch.cuda.synchronize()
                        e2e[g].append(e0.elapsed_time(e1))
            kern = kernel_times(prof)
            row = dict(batch=label, packets=m, fix_lengths=fix, compute_checksums=csum, payload_bytes=payload,
                       written_bytes=written, packets_in_error=counts[2], mean_packet_bytes=payload / m, groups={})
            head = pick(kern, ("ser_head_kernel",))  # one per call, the same work at both group sizes
            for g in (16, 64):
                mv = pick(kern, ("ser_move_kernel",), ("<%d," % g, "Li%dE" % g))
                fr = pick(kern, ("frame_kernel",), ("<%d>" % g, "Li%dE" % g))
                if len(mv) != a.runs or len(fr) != a.runs or len(head) != 2 * a.runs:
                    row["kernel_names_seen"] = sorted(kern)[:40]
                    continue
                hd = statistics.median(head)
                w = [x + hd for x in mv]
                moved = payload + written
                row["groups"][str(g)] = dict(
                    move_ms=spread(mv), head_ms=spread(head), write_ms=spread(w), frame_ms=spread(fr),
                    e2e_ms=spread(e2e[g]),
                    write_GBps=spread([moved / (x * 1e6) for x in w]),
                    frame_GBps=spread([(2 * payload + 16 * m) / (x * 1e6) for x in fr]),
                    write_Mpps=spread([m / (x * 1e3) for x in w]),
                    ratio_move_over_frame=spread([x / y for x, y in zip(mv, fr)]),
                    ratio_write_over_frame=spread([x / y for x, y in zip(w, fr)]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del out
        return rows

    for cfg in (synth.C2_UDP64, synth.C3_TCP1500, synth.C4_IMIX):
        d, o, c = synth.device_batch(cfg, 0, n)
        res["rows"] += measure(d, o, c, n, synth.NAMES[cfg], OPTS)
        if cfg == synth.C3_TCP1500:
            m = n - 16
            for caplen in (128, 256, 512, 768, 1024, 1280, 1500):
                c2 = torch.full_like(c, caplen)
                for r in measure(d, o, c2, m, "decoded", [(1, 1)]):
                    res["crossover"].append(r)
            for caplen in (256, 1024, 1500, 2048, 3072, 4096, 9000):
                c2 = torch.full_like(c, caplen)  # stretched over the packets that follow: bytes of the same allocation
                for r in measure(d, o, c2, m, "raw", [(0, 1)], decoded=False):
                    res["crossover"].append(r)
        del d, o, c
        torch.cuda.empty_cache()
    for series in ("decoded", "raw"):
        rows = [r for r in res["crossover"] if r["batch"] == series and len(r["groups"]) == 2]
        w16 = [r["mean_packet_bytes"] for r in rows
               if r["groups"]["16"]["write_ms"]["median"] <= r["groups"]["64"]["write_ms"]["median"]]
        w64 = [r["mean_packet_bytes"] for r in rows
               if r["groups"]["16"]["write_ms"]["median"] > r["groups"]["64"]["write_ms"]["median"]]
        res["crossover_%s" % series] = dict(wins16=w16, wins64=w64)
    res["chosen_threshold"] = a.threshold
    L.gpk_capwriter_destroy(h)
    ser.close()
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
