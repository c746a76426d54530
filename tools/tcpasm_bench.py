#!/usr/bin/env python3
"""Measure the device TCP reassembly (include/gpk_tcpasm.h) on one GPU.

(a) mixed: tests/tcpasmcases.random_traffic builds a template of --template
    connections (interleaved keys, reordering, loss, duplication, overlap,
    IPv4 / IPv6 / VLAN), numpy repeats it --repeat times with the replica number
    written into an address (so every replica has its own keys; the IPv4 header
    checksum is not refreshed, which reassembly does not read). Uploaded once.
    Reported: milliseconds for decode+layouts, grouping, and of
    gpk_tcpasm_batch its plan (prep + plan kernels), scans (+ finish, pending)
    and emit (records + bytes) kernels, end to end (group + assemble),
    packets/s, the bytes the mover writes and its GB/s, beside a
    device-to-device memcpy of the same byte count (the ceiling, not a target),
    interleaved with it in this process.
(b) elephant: one connection of --elephant in-order segments (the wave retires
    64 per step), and the same with every adjacent pair swapped (every second
    segment is queued and popped by the next: one packet per step).
Kernel times come from the profiler's device timeline, one sample per run;
medians and min..max over --runs timed runs after --warmup.
Every batch also gets a `timed` row (tools/reasm_time_ab.py): gpk_tcpasm_batch
and gpk_tcpasm_batch_timed (timestamps in, lastSeen kept, no FlushOlderThan) on
the same batch, interleaved, with the ratio of their plan times.

  python tools/tcpasm_bench.py --out profiles/tcpasm.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_mixed(conns, repeat, seed):
    import pktutil
    import tcpasmcases as TC
    pk = TC.random_traffic(seed, conns)
    data, off, cap = pktutil.pack(pk)
    T = int(off[-1] + cap[-1])
    big = np.tile(data[:T], repeat)
    offs = (off[None, :] + (np.arange(repeat, dtype=np.uint64) * np.uint64(T))[:, None]).reshape(-1)
    caps = np.tile(cap, repeat)
    rep = np.repeat(np.arange(repeat, dtype=np.uint32), len(off))
    at = offs.astype(np.int64) + 14 + 16  # inside an address of every frame kind: part of the key
    big[at + 1] = (rep >> 8).astype(np.uint8)
    big[at + 2] = (rep & 0xFF).astype(np.uint8)
    return np.concatenate([big, np.zeros(64, np.uint8)]), offs, caps


def build_elephant(n, payload, swapped):
    import tcpasmcases as TC
    syn = np.frombuffer(TC.seg(999, TC.SYN), np.uint8)
    one = np.frombuffer(TC.seg(0, 0, bytes(range(256)) * (payload // 256 + 1))[:54 + payload], np.uint8).copy()
    one[16:18] = [(40 + payload) >> 8, (40 + payload) & 255]  # IPv4 Total Length of the cut frame
    L = len(one)
    body = np.tile(one, n).reshape(n, L)
    order = np.arange(n)
    if swapped:
        order[1:n - 1:2], order[2:n:2] = np.arange(2, n, 2)[:len(order[1:n - 1:2])], np.arange(1, n - 1, 2)[:len(order[2:n:2])]
    seq = (1000 + order.astype(np.uint64) * payload) & 0xFFFFFFFF
    for k in range(4):
        body[:, 38 + k] = (seq >> (24 - 8 * k)).astype(np.uint8)
    data = np.concatenate([syn, body.reshape(-1), np.zeros(64, np.uint8)])
    off = np.concatenate([[0], len(syn) + np.arange(n, dtype=np.uint64) * L]).astype(np.uint64)
    cap = np.concatenate([[len(syn)], np.full(n, L)]).astype(np.uint32)
    return data, off, cap


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def measure(torch, profile, activities, ctx, parser, flows, batch, a, memcpy):
    data, off, cap = batch
    n = len(off)
    d = torch.from_numpy(data).cuda()
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    c = torch.from_numpy(cap.astype(np.int32)).cuda()
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    flw = torch.zeros(n * 3, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream()
    g, asm = flows.Grouper(n), flows.Assembler(n)
    out_data = torch.empty(d.numel() + 16, dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    def one():
        ev[0].record()
        ctx.decode_device(parser, d, o, c, rec, None, flw, lay, stream=st)
        ev[1].record()
        groups = g.group(d, o, c, rec, lay, kind=flows.CONNECTION, stream=st)
        ev[2].record()
        out = asm.assemble(d, o, c, rec, lay, groups, max_pages=a.max_pages, flush=True, out_data=out_data,
                           data_cap=d.numel(), stream=st)
        ev[3].record()
        return groups, out

    groups, out = one()
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    nbytes = counts[2]
    mc_src, mc_dst = d[:nbytes], torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")[:nbytes]
    for _ in range(a.warmup):
        one()
        if memcpy:
            mc_dst.copy_(mc_src)
    torch.cuda.synchronize()
    t = dict(decode=[], group=[], assemble=[], end_to_end=[], memcpy=[])
    with profile(activities=activities) as prof:
        for _ in range(a.runs):  # the movers interleaved, so drift hits both alike
            one()
            ev[4].record()
            if memcpy:
                mc_dst.copy_(mc_src)
            e5 = torch.cuda.Event(enable_timing=True)
            e5.record()
            torch.cuda.synchronize()
            t["decode"].append(ev[0].elapsed_time(ev[1]))
            t["group"].append(ev[1].elapsed_time(ev[2]))
            t["assemble"].append(ev[2].elapsed_time(ev[3]))
            t["end_to_end"].append(ev[1].elapsed_time(ev[3]))
            t["memcpy"].append(ev[4].elapsed_time(e5))
    kern = {}
    for e in prof.events():
        if "cuda" not in str(getattr(e, "device_type", "")).lower():
            continue
        us = getattr(e, "device_time", None)
        if us is None:
            us = getattr(e, "cuda_time", 0.0)
        kern.setdefault(e.name, []).append(us / 1000.0)

    def per_run(*pieces):
        tot = None
        for name, xs in kern.items():
            if any(p in name for p in pieces) and len(xs) % a.runs == 0 and xs:
                k = len(xs) // a.runs
                s = [sum(xs[i * k:(i + 1) * k]) for i in range(a.runs)]
                tot = s if tot is None else [x + y for x, y in zip(tot, s)]
        return tot

    plan, emit = per_run("prep_kernel", "plan_kernel"), per_run("emit_kernel")
    fin = per_run("finish_kernel", "pend_kernel")
    if not memcpy:
        del t["memcpy"]
    res = dict(packets=n, batch_bytes=int(d.numel()), groups=int(groups["counts"][0].item()), streams=counts[0],
               chunks=counts[1], stream_bytes=nbytes, pending=counts[3], ms={k: spread(v) for k, v in t.items()})
    if plan and emit:
        scans = [x - p - q for x, p, q in zip(t["assemble"], plan, emit)]
        res["ms"].update(plan=spread(plan), emit=spread(emit), scans_and_finish=spread(scans))
        if fin:
            res["ms"]["finish_and_pending"] = spread(fin)
        res["emit_GBps"] = spread([nbytes / (x * 1e6) for x in emit])
        res["plan_packets_per_s"] = n / (statistics.median(plan) / 1e3)
    else:
        res["kernel_times"] = "the profiler returned no device timeline for the kernels"
        res["kernel_names_seen"] = sorted(kern)[:40]
    if memcpy:
        res["memcpy_GBps"] = spread([nbytes / (x * 1e6) for x in t["memcpy"]])
    res["packets_per_s"] = n / (statistics.median(t["end_to_end"]) / 1e3)
    import reasm_time_ab
    seen = torch.arange(n, dtype=torch.int64, device="cuda") * 1000 + 1700000000 * 10 ** 9

    def call(**kw):
        return asm.assemble(d, o, c, rec, lay, groups, max_pages=a.max_pages, flush=True, out_data=out_data,
                            data_cap=d.numel(), stream=st, **kw)

    res["timed"] = reasm_time_ab.ab_rows(torch, profile, activities, call, lambda: call(seen=seen), a.runs, a.warmup,
                                         shared=("prep_kernel",),
                                         untimed_only=("plan_kernel<true, false>", "plan_kernel<false, false>",
                                                       "plan_kernelILb1ELb0E", "plan_kernelILb0ELb0E"),
                                         timed_only=("plan_kernel<true, true>", "plan_kernel<false, true>",
                                                     "plan_kernelILb1ELb1E", "plan_kernelILb0ELb1E"))
    g.close()
    asm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--template", type=int, default=4000)
    ap.add_argument("--repeat", type=int, default=25)
    ap.add_argument("--elephant", type=int, default=1 << 18)
    ap.add_argument("--payload", type=int, default=512)
    ap.add_argument("--max-pages", type=int, default=0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from torch.profiler import ProfilerActivity, profile

    import flowcases
    from configs import device_parser
    from gopacket_amd import engine, flows

    ctx = engine.Context(0)
    parser = device_parser(flowcases.DEFRAG_PARSER)
    act = [ProfilerActivity.CPU, ProfilerActivity.CUDA]
    props = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=props.gcnArchName, compute_units=props.multi_processor_count,
               max_pages=a.max_pages, flush=True,
               method="one process, %d timed runs after %d warm-up; stage times from stream events, kernel times "
                      "from the profiler's device timeline; medians with min..max; the memcpy interleaved per run"
                      % (a.runs, a.warmup))
    res["mixed"] = measure(torch, profile, act, ctx, parser, flows, build_mixed(a.template, a.repeat, a.seed), a, True)
    res["elephant_in_order"] = measure(torch, profile, act, ctx, parser, flows,
                                       build_elephant(a.elephant, a.payload, False), a, False)
    res["elephant_pairs_swapped"] = measure(torch, profile, act, ctx, parser, flows,
                                            build_elephant(a.elephant, a.payload, True), a, False)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
