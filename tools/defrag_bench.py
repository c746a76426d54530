#!/usr/bin/env python3
"""Measure the device reassembly (include/gpk_defrag.h) on one GPU.

Input: UDP datagrams of 3-9 KB cut at MTU 1500, a few percent reordered,
duplicated or dropped, keys interleaved: tests/defragcases.random_traffic
builds a template of --template datagrams, numpy repeats it --repeat times
with the replica number written into the destination address (so every replica
has its own keys; the IPv4 header checksum is not refreshed, which reassembly
does not read). Uploaded once.

Reported: milliseconds for decode+layouts, grouping, and of gpk_defrag_batch
its plan (prep + plan kernels), scans (+ finish) and copy kernels, end to end
(group + defrag), datagrams/s, the bytes the copy kernel moves and its GB/s.
Yardsticks for the copy kernel, interleaved with it in this process:
gpk_pack_batch's byte kernel moving the keyed packets of the same batch, and a
device-to-device memcpy of the copy's byte count (the ceiling, not a target).
Kernel times come from the profiler's device timeline, one sample per run;
medians and min..max over --runs timed runs after --warmup.
A `timed` row follows (tools/reasm_time_ab.py): gpk_defrag_batch and
gpk_defrag_batch_timed (timestamps in, LastSeen out, no discard) on the same
batch, interleaved, with the ratio of their plan times.

  python tools/defrag_bench.py --out profiles/defrag.json
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


def build_batch(template_datagrams, repeat, seed):
    import defragcases as DC
    import pktutil
    pk = DC.random_traffic(seed, template_datagrams, lo=3000, hi=9000, per=1480, window=60, dup=0.02, drop=0.01,
                           corrupt=0.0)
    data, off, cap = pktutil.pack(pk)
    T = int(off[-1] + cap[-1])
    data = data[:T]
    big = np.tile(data, repeat)
    offs = (off[None, :] + (np.arange(repeat, dtype=np.uint64) * np.uint64(T))[:, None]).reshape(-1)
    caps = np.tile(cap, repeat)
    rep = np.repeat(np.arange(repeat, dtype=np.uint32), len(off))
    at = offs.astype(np.int64) + 14 + 16  # the IPv4 destination address
    big[at + 1] = (rep >> 8).astype(np.uint8)
    big[at + 2] = (rep & 0xFF).astype(np.uint8)
    return np.concatenate([big, np.zeros(64, np.uint8)]), offs, caps


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--template", type=int, default=4000)
    ap.add_argument("--repeat", type=int, default=100)
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

    data, off, cap = build_batch(a.template, a.repeat, a.seed)
    n = len(off)
    d = torch.from_numpy(data).cuda()
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    c = torch.from_numpy(cap.astype(np.int32)).cuda()
    ctx = engine.Context(0)
    parser = device_parser(flowcases.DEFRAG_PARSER)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    flw = torch.zeros(n * 3, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream()
    g, df = flows.Grouper(n), flows.Defragmenter(n)
    out_data = torch.empty(d.numel() + 16, dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    def one():
        ev[0].record()
        ctx.decode_device(parser, d, o, c, rec, None, flw, lay, stream=st)
        ev[1].record()
        groups = g.group(d, o, c, rec, lay, kind=flows.DEFRAG, stream=st)
        ev[2].record()
        out = df.defrag(d, o, c, rec, lay, groups, out_data=out_data, data_cap=d.numel(), stream=st)
        ev[3].record()
        return groups, out

    groups, out = one()
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    keyed = torch.nonzero(groups["group_of"] >= 0).flatten().to(torch.int32)
    keyed_bytes = int(c.index_select(0, keyed.long()).sum(dtype=torch.int64).item())
    copy_bytes = counts[2]
    pack_out = torch.empty(keyed_bytes + 16, dtype=torch.uint8, device="cuda")
    mc_src, mc_dst = d[:copy_bytes], torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")

    def pack():
        return flows.pack_batch(d, o, c, keyed, total_bytes=keyed_bytes, stream=st)

    for _ in range(a.warmup):
        one()
        pack()
        mc_dst.copy_(mc_src)
    torch.cuda.synchronize()
    t = dict(decode=[], group=[], defrag=[], end_to_end=[], memcpy=[])
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(a.runs):  # the movers interleaved, so drift hits all alike
            one()
            pack()
            ev[4].record()
            mc_dst.copy_(mc_src)
            e5 = torch.cuda.Event(enable_timing=True)
            e5.record()
            torch.cuda.synchronize()
            t["decode"].append(ev[0].elapsed_time(ev[1]))
            t["group"].append(ev[1].elapsed_time(ev[2]))
            t["defrag"].append(ev[2].elapsed_time(ev[3]))
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

    plan = per_run("prep_kernel", "plan_kernel")
    copy = per_run("copy_kernel")
    packk = per_run("pack_bytes_kernel")
    fin = per_run("finish_kernel")
    res = dict(
        device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
        compute_units=torch.cuda.get_device_properties(0).multi_processor_count, fragments=n, batch_bytes=int(d.numel()), datagrams=counts[0],
        pending=counts[1], groups=int(groups["counts"][0].item()), copy_bytes=copy_bytes, pack_bytes=keyed_bytes,
        method="one process, movers interleaved per run, %d timed runs after %d warm-up; stage times from events, "
               "kernel times from the profiler's device timeline; medians with min..max" % (a.runs, a.warmup),
        ms={k: spread(v) for k, v in t.items()},
    )
    if plan and copy and packk:
        scans = [x - p - q for x, p, q in zip(t["defrag"], plan, copy)]
        res["ms"].update(plan=spread(plan), copy=spread(copy), scans_and_finish=spread(scans),
                         pack_bytes_kernel=spread(packk))
        if fin:
            res["ms"]["finish"] = spread(fin)
        res["copy_GBps"] = spread([copy_bytes / (x * 1e6) for x in copy])
        res["pack_GBps"] = spread([keyed_bytes / (x * 1e6) for x in packk])
    else:
        res["kernel_times"] = "the profiler returned no device timeline for the kernels"
        res["kernel_names_seen"] = sorted(kern)[:40]
    res["memcpy_GBps"] = spread([copy_bytes / (x * 1e6) for x in t["memcpy"]])
    res["datagrams_per_s"] = counts[0] / (statistics.median(t["end_to_end"]) / 1e3)
    import reasm_time_ab
    seen = torch.arange(n, dtype=torch.int64, device="cuda") * 1000 + 1700000000 * 10 ** 9

    def call(**kw):
        return df.defrag(d, o, c, rec, lay, groups, out_data=out_data, data_cap=d.numel(), stream=st, **kw)

    res["timed"] = reasm_time_ab.ab_rows(torch, profile, [ProfilerActivity.CPU, ProfilerActivity.CUDA], call,
                                         lambda: call(seen=seen), a.runs, a.warmup,
                                         shared=("prep_kernel", "plan_kernel"),
                                         timed_only=("mark_kernel", "key_kernel", "drop_kernel", "seen_kernel"))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
