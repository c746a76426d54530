#!/usr/bin/env python3
"""Measure gpk_tunnel_batch (include/gpk_tunnel.h) and the decode of its
zero-copy inner batch on one GPU.

Input: 1 Mi-packet batches of the C4 (IMIX) and C3 (1500-byte TCP) shapes
generated in HBM (gopacket_amd.synth), each packet encapsulated on the device
in Ethernet / IPv4 / UDP 4789 / VXLAN (50 bytes), and once more with only 1
packet in 64 encapsulated. Per batch, median (min..max) over --runs timed runs
after --warmup, the calls alternating inside every run so drift hits all alike:
  peel          the whole gpk_tunnel_batch call between two events, and its
                kernels from the profiler's device timeline (classify, the scan,
                scatter)
  inner decode  gpk_decode_batch of the inner class
                  zero_copy    on in_offsets / in_caplens as the peel wrote them
                  pack         gpk_pack_batch of those slices
                  packed       the decode of the packed copy (the same packets,
                               never encapsulated, dense)
                pack + packed is the alternative to zero_copy
GRE sum: the C3 batch behind Ethernet / IPv4 / GRE with the C bit; the sum
kernels' device time and GB/s over the summed bytes against
gpk_capwrite_batch's frame_kernel (pcap) over the same packets. The crossover
table runs the sum with every slice on the 16-lane and on the 64-lane kernel
over uniform slice lengths; GPK_TUN_SUM_GROUP_BYTES is read off it.

  python tools/tunnel_bench.py --out profiles/tunnel.json
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# this pass's instantiation of a kernel template of csrc/gpk_postpass.h, by its demangled name
OWN = r"\b%s_kernel<.*TunnelPass>"


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

    L = _lib.lib()
    n = a.packets
    prop = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               packets=n, sum_group_bytes=_lib.TUN_SUM_GROUP_BYTES,
               method="one process, calls alternating inside every run, %d timed runs after %d warm-up; call times "
                      "between events, kernel times from the profiler's device timeline; medians with min..max"
                      % (a.runs, a.warmup), rows=[], gre_sum=None, crossover=[])
    ctx = engine.Context(0)
    kinds = [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP,
             _lib.DEC_PAYLOAD]
    parser = engine.ParserConfig(17, kinds)
    det = flows.Detunneler(n)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    rec2 = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")

    def encapsulate(d, o, c, header, len_at, every=1):
        """header (bytes) in front of every `every`-th packet; len_at: (byte offset, constant) pairs
        of big-endian 16-bit length fields = constant + the packet's length. One gpk_pack_batch of
        the 2n pieces header_i, packet_i."""
        m = o.numel()
        hl = len(header)
        h = torch.tensor(list(header), dtype=torch.uint8, device="cuda").repeat(m, 1)
        for at, k in len_at:
            v = c + k
            h[:, at] = (v >> 8).to(torch.uint8)
            h[:, at + 1] = (v & 255).to(torch.uint8)
        tun = (torch.arange(m, device="cuda") % every) == 0
        cat = torch.cat([h.flatten(), d])
        po = torch.stack([torch.arange(m, device="cuda", dtype=torch.int64) * hl, o + m * hl], 1).flatten()
        pc = torch.stack([torch.where(tun, hl, 0).int(), c], 1).flatten()
        od, oo, oc = flows.pack_batch(cat, po, pc, torch.arange(2 * m, device="cuda", dtype=torch.int32))
        pad = torch.zeros(od.numel() + 32, dtype=torch.uint8, device="cuda")
        pad[:od.numel()] = od
        return pad, oo[0::2].contiguous(), (oc[0::2] + oc[1::2]).contiguous()

    mac = bytes(range(1, 13))
    ip = lambda proto: struct.pack(">BBHHHBBH", 0x45, 0, 0, 1, 0, 64, proto, 0) + bytes([10, 0, 0, 1, 10, 0, 0, 2])  # noqa: E731
    vx_hdr = mac + b"\x08\x00" + ip(17) + struct.pack(">HHHH", 50000, 4789, 0, 0) + bytes([8, 0, 0, 0, 0, 0, 7, 0])
    gre_hdr = mac + b"\x08\x00" + ip(47) + bytes([0x80, 0, 8, 0, 0x12, 0x34, 0, 0])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    for cfg in (synth.C4_IMIX, synth.C3_TCP1500):
        d0, o0, c0 = synth.device_batch(cfg, 0, n)
        for every in (1, 64):
            d, o, c = encapsulate(d0, o0, c0, vx_hdr, [(16, 36), (38, 16)], every)
            ctx.decode_device(parser, d, o, c, rec, err, fl, lay)
            out = det.peel(ctx, d, o, c, rec, lay, parser)
            torch.cuda.synchronize()
            cs = out["class_start"].cpu().tolist()
            m = cs[1] - cs[0]
            io, ic = out["in_offsets"][cs[0]:cs[1]], out["in_caplens"][cs[0]:cs[1]]
            inner_bytes = int(ic.sum(dtype=torch.int64).item())
            order = torch.arange(m, device="cuda", dtype=torch.int32)
            pd, po, pc = flows.pack_batch(d, io, ic, order, total_bytes=inner_bytes)

            def peel():
                det.peel(ctx, d, o, c, rec, lay, parser, out=out)

            def zero():
                ctx.decode_device(parser, d, io, ic, rec2, err, fl)

            def pack():
                flows.pack_batch(d, io, ic, order, total_bytes=inner_bytes)

            def packed():
                ctx.decode_device(parser, pd, po, pc, rec2, err, fl)

            calls = dict(peel=peel, zero_copy=zero, pack=pack, packed=packed)
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
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:  # the peel alone:
                for _ in range(a.runs):                                                      # its scan's kernels
                    peel()                                                                   # share names with
                    torch.cuda.synchronize()                                                 # gpk_pack_batch's
            kern = kernel_times(prof)
            row = dict(batch=synth.NAMES[cfg], tunnelled_one_in=every, packets=n, inner_packets=m,
                       batch_bytes=int(c.sum(dtype=torch.int64).item()), inner_bytes=inner_bytes,
                       peel_ms=spread(t["peel"]), peel_Mpps=spread([n / (x * 1e3) for x in t["peel"]]),
                       peel_kernels_ms=dict(classify=per_run(kern, a.runs, OWN % "classify"),
                                            scatter=per_run(kern, a.runs, OWN % "scatter"),
                                            scan=per_run(kern, a.runs, "scan",
                                                         r"\bfinish_kernel<%d>" % _lib.TUN_NCLASS)),
                       inner_decode_ms=dict(zero_copy=spread(t["zero_copy"]), pack=spread(t["pack"]),
                                            packed=spread(t["packed"]),
                                            pack_plus_packed=spread([x + y for x, y in zip(t["pack"], t["packed"])])),
                       zero_copy_over_pack_plus_packed=spread(
                           [z / (x + y) for z, x, y in zip(t["zero_copy"], t["pack"], t["packed"])]),
                       zero_copy_over_packed=spread([z / y for z, y in zip(t["zero_copy"], t["packed"])]))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del d, o, c, pd, po, pc, out

    # ---- the GRE sum against the capture writer's framing kernel
    d0, o0, c0 = synth.device_batch(synth.C3_TCP1500, 0, n)
    d, o, c = encapsulate(d0, o0, c0, gre_hdr, [(16, 28)])
    h = ctypes.c_void_p()
    _lib.check(L.gpk_capwriter_create(ctypes.byref(h), _lib.CAPW_PCAP_NANO, 0, n))
    ci = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
    ci[:, 0] = 1600000000
    ci[:, 5] = -1
    boff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    stt = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream()

    def sum_vs_frame(d, o, c_now, threshold, frame=True):
        n = o.numel()
        ctx.decode_device(parser, d, o, c_now, rec, err, fl, lay)
        det.set_sum_threshold(threshold)
        out = det.peel(ctx, d, o, c_now, rec, lay, parser)
        torch.cuda.synchronize()
        sums = int(out["counts"][7].item())
        payload = int(c_now.sum(dtype=torch.int64).item())
        summed = payload - 34 * n
        if frame:
            cap = payload + 128 * n
            buf = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
            ci[:, 3] = c_now
            b = _lib.Batch(d.data_ptr(), o.data_ptr(), c_now.data_ptr(), n, d.numel())
            op = _lib.CapwriteOpts(0, 0, 0)

        def fr():
            _lib.check(L.gpk_capwrite_batch(h, ctypes.byref(b), None, n, ci.data_ptr(), None, None, ctypes.byref(op),
                                            buf.data_ptr(), cap, boff.data_ptr(), stt.data_ptr(), cnt.data_ptr(),
                                            st.cuda_stream))
        for _ in range(a.warmup):
            det.peel(ctx, d, o, c_now, rec, lay, parser, out=out)
            if frame:
                fr()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.runs):
                det.peel(ctx, d, o, c_now, rec, lay, parser, out=out)
                if frame:
                    fr()
                torch.cuda.synchronize()
        kern = kernel_times(prof)
        s16 = [x for k, v in kern.items() if re.search(OWN % "sum16", k) for x in v]
        s64 = [x for k, v in kern.items() if re.search(OWN % "sum64", k) for x in v]
        f = [x for k, v in kern.items() if "frame_kernel" in k for x in v]
        return sums, summed, payload, s16, s64, f

    sums, summed, payload, s16, s64, f = sum_vs_frame(d, o, c, _lib.TUN_SUM_GROUP_BYTES)
    both = [x + y for x, y in zip(s16, s64)] if len(s16) == len(s64) else []
    res["gre_sum"] = dict(batch="C3-tcp1500 behind Ethernet/IPv4/GRE (C bit)", sums_computed=sums, summed_bytes=summed,
                          sum16_ms=spread(s16), sum64_ms=spread(s64), sum_ms=spread(both),
                          sum_GBps=spread([summed / (x * 1e6) for x in both]), frame_ms=spread(f),
                          frame_GBps_read_plus_written=spread([(2 * payload + 16 * n) / (x * 1e6) for x in f]),
                          frame_GBps_read=spread([payload / (x * 1e6) for x in f]))
    print(json.dumps(res["gre_sum"]), flush=True)
    # uniform slices: nx packets of Ethernet / IPv4 / GRE (C bit) + random bytes at a fixed stride
    del d, o, c, d0, o0, c0
    nx = min(n, 1 << 17)
    for ln in (64, 128, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2560, 3072, 4096, 8192):
        stride = (ln + 34 + 15) // 16 * 16 + 16
        dx = torch.randint(0, 256, (nx * stride + 32,), dtype=torch.uint8, device="cuda")
        ox = torch.arange(nx, device="cuda", dtype=torch.int64) * stride + 3
        hdr = bytearray(gre_hdr)
        hdr[16:18] = struct.pack(">H", 20 + ln)
        idx = (ox[:, None] + torch.arange(42, device="cuda")[None, :]).flatten()
        dx[idx] = torch.tensor(list(hdr), dtype=torch.uint8, device="cuda").repeat(nx)
        cx = torch.full((nx,), ln + 34, dtype=torch.int32, device="cuda")
        sums, summed, _, a16, _, _ = sum_vs_frame(dx, ox, cx, 1 << 31, frame=False)
        _, _, _, _, b64, _ = sum_vs_frame(dx, ox, cx, 1, frame=False)
        assert sums == nx, (sums, nx)
        row = dict(slice_bytes=ln, packets=nx, lanes16_ms=spread(a16), lanes64_ms=spread(b64),
                   lanes16_GBps=spread([summed / (x * 1e6) for x in a16]),
                   lanes64_GBps=spread([summed / (x * 1e6) for x in b64]))
        res["crossover"].append(row)
        print(json.dumps(row), flush=True)
        del dx, ox, cx, idx
    det.set_sum_threshold(_lib.TUN_SUM_GROUP_BYTES)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
