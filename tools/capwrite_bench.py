#!/usr/bin/env python3
"""Measure the device framing of capture files (include/gpk_capwrite.h) on one GPU.

Input: synthetic batches generated in HBM (gopacket_amd.synth), each written
whole and with an irregular selection of about 10 % of its packets as `order`:
the C4 IMIX mix (about 16 Mi packets) and C3's 1500-byte packets (about 4 Mi);
C2's 64-byte packets are added as the small end of the block-size range. The
output format is pcapng (28-byte head, padding, trailer).

Reported per batch and selection, median (min..max) over --runs timed runs
after --warmup, the movers alternating inside every run so drift hits all
alike:
  frame16 / frame64   the framing kernel at 16 and at 64 lanes per packet:
                      bytes written per second (kernel time from the profiler's
                      device timeline)
  pack                gpk_pack_batch's byte kernel on the same selection
  memcpy              a device-to-device copy of the framing's byte count (the
                      ceiling, not a target)
  e2e16 / e2e64       the whole gpk_capwrite_batch call (size kernel, scan,
                      counts, framing) between two events
  host                gpk_capwrite_batch_host on one thread over a prefix of
                      --host-packets packets
The host's group-size threshold (kGroup16MaxMean in gpk_capwrite.hip) is read
off the frame16 / frame64 columns against the batches' mean block sizes.

  python tools/capwrite_bench.py --out profiles/capwrite.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def crossover(a, L, h, b, d, o, c, ci, n, st):
    """The framing kernel at both group sizes over uniform blocks of every
    size: the 1500-byte batch with its capture lengths cut (or stretched over
    the packets that follow, which are bytes of the same allocation; the last
    packets are left out so that nothing reaches past it)."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    from gopacket_amd import _lib
    m = n - 16
    rows = []
    for caplen in (128, 256, 384, 512, 768, 1024, 1280, 1500, 2048, 3072, 4096, 9000):
        c2 = torch.full_like(c, caplen)
        ci[:, 3] = c2
        b2 = _lib.Batch(d.data_ptr(), o.data_ptr(), c2.data_ptr(), n, d.numel())
        cap = (caplen + 36) * m
        out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
        boff = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        stt = torch.empty(m, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")

        def frame(group):
            op = _lib.CapwriteOpts(0, 0, group)
            _lib.check(L.gpk_capwrite_batch(h, ctypes.byref(b2), None, m, ci.data_ptr(), None, None, ctypes.byref(op),
                                            out.data_ptr(), cap, boff.data_ptr(), stt.data_ptr(), cnt.data_ptr(),
                                            st.cuda_stream))

        for _ in range(a.warmup):
            frame(16)
            frame(64)
        torch.cuda.synchronize()
        counts = cnt.cpu().tolist()
        assert counts[0] == m and counts[3] == 0, counts
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(a.runs):
                frame(16)
                frame(64)
            torch.cuda.synchronize()
        ms = {16: [], 64: []}
        for e in prof.events():
            if "frame_kernel" in e.name and "cuda" in str(getattr(e, "device_type", "")).lower():
                us = getattr(e, "device_time", None)
                if us is None:
                    us = getattr(e, "cuda_time", 0.0)
                ms[16 if ("<16>" in e.name or "Li16E" in e.name) else 64].append(us / 1000.0)
        row = dict(block_bytes=counts[1] / m, packets=m,
                   GBps={str(g): spread([counts[1] / (x * 1e6) for x in ms[g]]) for g in (16, 64) if ms[g]})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out
    ci[:, 3] = c
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--imix-packets", type=int, default=1 << 24)
    ap.add_argument("--big-packets", type=int, default=1 << 22)
    ap.add_argument("--small-packets", type=int, default=1 << 24)
    ap.add_argument("--host-packets", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=int, default=1792,
                    help="kGroup16MaxMean of gpk_capwrite.hip, recorded next to the table it came from")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from torch.profiler import ProfilerActivity, profile

    from gopacket_amd import _lib, flows, synth

    L = _lib.lib()
    st = torch.cuda.current_stream()
    prop = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               format="pcapng",
               method="one process, movers alternating inside every run, %d timed runs after %d warm-up; kernel times "
                      "from the profiler's device timeline, e2e between events; medians with min..max" %
                      (a.runs, a.warmup), rows=[])

    for cfg, n in ((synth.C2_UDP64, a.small_packets), (synth.C4_IMIX, a.imix_packets),
                   (synth.C3_TCP1500, a.big_packets)):
        d, o, c = synth.device_batch(cfg, 0, n)
        ci = torch.zeros((n, 6), dtype=torch.int32, device="cuda")  # gpk_capture_info as int32 words
        ci[:, 0] = 1600000000
        ci[:, 2] = torch.arange(n, device="cuda", dtype=torch.int32) % 1000000000
        ci[:, 3] = c
        ci[:, 5] = -1
        idx = torch.arange(n, device="cuda", dtype=torch.int64)
        keep = ((idx * 2654435761) >> 7) % 10 == 0
        sel = torch.nonzero(keep).flatten().to(torch.int32)
        h = ctypes.c_void_p()
        _lib.check(L.gpk_capwriter_create(ctypes.byref(h), _lib.CAPW_PCAPNG, 0, n))
        _lib.check(L.gpk_capwriter_set_interfaces(h, 1))
        b = _lib.Batch(d.data_ptr(), o.data_ptr(), c.data_ptr(), n, d.numel())
        for label, order in (("whole", None), ("select10", sel)):
            m = n if order is None else order.numel()
            payload = int((c if order is None else c.index_select(0, order.long())).sum(dtype=torch.int64).item())
            cap = payload + 36 * m
            out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
            boff = torch.empty(m + 1, dtype=torch.int64, device="cuda")
            stt = torch.empty(m, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            every = torch.arange(n, device="cuda", dtype=torch.int32) if order is None else order

            def frame(group):
                op = _lib.CapwriteOpts(0, 0, group)
                _lib.check(L.gpk_capwrite_batch(h, ctypes.byref(b), order.data_ptr() if order is not None else None,
                                                m, ci.data_ptr(), None, None, ctypes.byref(op), out.data_ptr(), cap,
                                                boff.data_ptr(), stt.data_ptr(), cnt.data_ptr(), st.cuda_stream))

            def pack():
                return flows.pack_batch(d, o, c, every, total_bytes=payload, stream=st)

            frame(0)
            torch.cuda.synchronize()
            counts = cnt.cpu().tolist()
            assert counts[0] == m and counts[2] == 0 and counts[3] == 0, counts
            written = counts[1]
            mc_src = d[:min(written, d.numel())]
            if mc_src.numel() < written:  # 64-byte packets: the framed output is larger than the batch
                mc_src = out[:written]
            mc_dst = torch.empty(written, dtype=torch.uint8, device="cuda")
            for _ in range(a.warmup):
                frame(16)
                frame(64)
                pack()
                mc_dst.copy_(mc_src)
            torch.cuda.synchronize()
            t = dict(e2e16=[], e2e64=[], memcpy=[])
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(a.runs):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                    ev[0].record()
                    frame(16)
                    ev[1].record()
                    frame(64)
                    ev[2].record()
                    pack()
                    ev[3].record()
                    ev[4].record()
                    mc_dst.copy_(mc_src)
                    ev[5].record()
                    torch.cuda.synchronize()
                    t["e2e16"].append(ev[0].elapsed_time(ev[1]))
                    t["e2e64"].append(ev[1].elapsed_time(ev[2]))
                    t["memcpy"].append(ev[4].elapsed_time(ev[5]))
            kern = {}
            for e in prof.events():
                if "cuda" not in str(getattr(e, "device_type", "")).lower():
                    continue
                us = getattr(e, "device_time", None)
                if us is None:
                    us = getattr(e, "cuda_time", 0.0)
                kern.setdefault(e.name, []).append(us / 1000.0)

            def per_run(*pieces):
                for name, xs in kern.items():
                    if all(any(q in name for q in p) for p in pieces) and xs and len(xs) % a.runs == 0:
                        k = len(xs) // a.runs
                        return [sum(xs[i * k:(i + 1) * k]) for i in range(a.runs)]
                return None

            f16 = per_run(("frame_kernel",), ("<16>", "Li16E"))
            f64 = per_run(("frame_kernel",), ("<64>", "Li64E"))
            pk = per_run(("pack_bytes_kernel",))
            for piece in ("size_kernel", "counts_kernel"):  # both group sizes' calls: two launches per run
                xs = per_run((piece,))
                if xs:
                    t[piece + "_x2"] = xs
            row = dict(batch=synth.NAMES[cfg], selection=label, packets=m, batch_packets=n, payload_bytes=payload,
                       written_bytes=written, mean_block_bytes=written / m, batch_mean_packet_bytes=d.numel() / n,
                       ms={k: spread(v) for k, v in t.items()})
            gb = {}
            if f16 and f64 and pk:
                row["ms"].update(frame16=spread(f16), frame64=spread(f64), pack=spread(pk))
                gb = dict(frame16=spread([written / (x * 1e6) for x in f16]),
                          frame64=spread([written / (x * 1e6) for x in f64]),
                          pack=spread([payload / (x * 1e6) for x in pk]))
            else:
                row["kernel_names_seen"] = sorted(kern)[:40]
            gb["memcpy"] = spread([written / (x * 1e6) for x in t["memcpy"]])
            gb["e2e16"] = spread([written / (x * 1e6) for x in t["e2e16"]])
            gb["e2e64"] = spread([written / (x * 1e6) for x in t["e2e64"]])
            row["GBps"] = gb
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del out, mc_dst, mc_src
        if cfg == synth.C3_TCP1500:
            res["crossover"] = crossover(a, L, h, b, d, o, c, ci, n, st)
        L.gpk_capwriter_destroy(h)
        # the CPU baseline: one thread over a prefix of the same batch
        hn = min(a.host_packets, n)
        hd, ho, hc = synth.host_batch(cfg, 0, hn)
        hci = np.zeros(hn, _lib.CAPINFO_DTYPE)
        hci["ts_sec"], hci["length"], hci["link_type"] = 1600000000, hc, -1
        hh = ctypes.c_void_p()
        _lib.check(L.gpk_capwriter_create(ctypes.byref(hh), _lib.CAPW_PCAPNG, -1, 0))
        _lib.check(L.gpk_capwriter_set_interfaces(hh, 1))
        hcap = int(hc.sum()) + 36 * hn
        hout = np.empty(hcap, np.uint8)
        hboff, hst, hcnt = np.zeros(hn + 1, np.uint64), np.zeros(hn, np.int32), np.zeros(4, np.uint64)
        hb = _lib.Batch(hd.ctypes.data, ho.ctypes.data, hc.ctypes.data, hn, len(hd))
        ts = []
        for _ in range(4):  # the first run touches the output's pages
            t0 = time.perf_counter()
            _lib.check(L.gpk_capwrite_batch_host(hh, ctypes.byref(hb), None, hn, hci.ctypes.data, None, None, None,
                                                 hout.ctypes.data, hcap, hboff.ctypes.data, hst.ctypes.data,
                                                 hcnt.ctypes.data))
            ts.append(time.perf_counter() - t0)
        L.gpk_capwriter_destroy(hh)
        row = dict(batch=synth.NAMES[cfg], selection="host-prefix", packets=hn, written_bytes=int(hcnt[1]),
                   GBps=dict(host=spread([int(hcnt[1]) / (x * 1e9) for x in ts[1:]])))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del d, o, c, ci, hd, hout
        torch.cuda.empty_cache()
    cross = res.get("crossover", [])
    wins16 = [r["block_bytes"] for r in cross if r["GBps"]["16"]["median"] >= r["GBps"]["64"]["median"]]
    wins64 = [r["block_bytes"] for r in cross if r["GBps"]["16"]["median"] < r["GBps"]["64"]["median"]]
    if wins16 and wins64:
        res["crossover_between"] = [max(wins16), min(wins64)]  # kGroup16MaxMean lies between them
    res["chosen_threshold"] = a.threshold
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
