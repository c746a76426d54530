#!/usr/bin/env python3
"""Measure the device IPv6 reassembly (include/gpk_defrag6.h) on one GPU.

Input: tools/defrag_bench.py's mix rebuilt as IPv6 fragments: UDP datagrams of
3-9 KB cut into fragments of 1448 bytes, a few percent reordered, duplicated or
dropped, keys interleaved (tests/defrag6cases.random_traffic builds a template
of --template datagrams, numpy repeats it --repeat times with the replica
number written into the top byte of the Identification, so every replica has
its own keys). The equivalent IPv4 batch (tests/defragcases.random_traffic,
same sizes, seed, fragment size and rates) is built beside it. Uploaded once.

Reported: milliseconds for decode+layouts, grouping, and of gpk_defrag6_batch
its plan (prep + plan kernels), scans (+ finish) and move kernels, end to end
(group + defrag), datagrams/s, the bytes the mover writes and its GB/s.
Yardsticks for the mover, interleaved with it in this process: IPv4's
copy_kernel on the equivalent IPv4 batch, gpk_pack_batch's byte kernel moving
the keyed packets of the IPv6 batch, and a device-to-device memcpy of the
mover's byte count (the ceiling, not a target). Kernel times come from the
profiler's device timeline, one sample per run; medians and min..max over
--runs timed runs after --warmup. A `timed` row follows
(tools/reasm_time_ab.py): gpk_defrag6_batch and gpk_defrag6_batch_timed
(timestamps in, key times out, no discard) on the same batch, interleaved, with
the ratio of their plan times.

  python tools/defrag6_bench.py --out profiles/defrag6.json
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


def tile(pk, repeat, mark):
    """The template repeated, mark(big, packet offsets, replica numbers) making every replica's keys its own."""
    import pktutil
    data, off, cap = pktutil.pack(pk)
    T = int(off[-1] + cap[-1])
    big = np.tile(data[:T], repeat)
    offs = (off[None, :] + (np.arange(repeat, dtype=np.uint64) * np.uint64(T))[:, None]).reshape(-1)
    caps = np.tile(cap, repeat)
    rep = np.repeat(np.arange(repeat, dtype=np.uint32), len(off))
    mark(big, offs.astype(np.int64), rep)
    return np.concatenate([big, np.zeros(64, np.uint8)]), offs, caps


def build_batches(template_datagrams, repeat, seed):
    import defrag6cases as DC6
    import defragcases as DC4
    kw = dict(lo=3000, hi=9000, per=1448, window=60, dup=0.02, drop=0.01)

    def mark6(big, at, rep):  # Ethernet 14 + IPv6 40 + 4: the Identification's top byte (the template's is 0)
        big[at + 58] = rep.astype(np.uint8)

    def mark4(big, at, rep):  # the IPv4 destination address
        big[at + 14 + 17] = (rep >> 8).astype(np.uint8)
        big[at + 14 + 18] = (rep & 0xFF).astype(np.uint8)

    assert repeat <= 256
    v6 = tile(DC6.random_traffic(seed, template_datagrams, vlan_every=0, **kw), repeat, mark6)
    v4 = tile(DC4.random_traffic(seed, template_datagrams, corrupt=0.0, **kw), repeat, mark4)
    return v6, v4


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

    v6, v4 = build_batches(a.template, a.repeat, a.seed)
    ctx = engine.Context(0)
    parser = device_parser(flowcases.DEFRAG_PARSER)
    st = torch.cuda.current_stream()

    def upload(batch):
        data, off, cap = batch
        n = len(off)
        return dict(n=n, d=torch.from_numpy(data).cuda(), o=torch.from_numpy(off.astype(np.int64)).cuda(),
                    c=torch.from_numpy(cap.astype(np.int32)).cuda(),
                    rec=torch.zeros(n * 16, dtype=torch.uint8, device="cuda"),
                    lay=torch.zeros(n * 64, dtype=torch.uint8, device="cuda"),
                    flw=torch.zeros(n * 3, dtype=torch.int64, device="cuda"), g=flows.Grouper(n))

    b6, b4 = upload(v6), upload(v4)
    df6, df4 = flows.Defragmenter6(b6["n"]), flows.Defragmenter(b4["n"])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    def one6(out_data, cap):
        b = b6
        ev[0].record()
        ctx.decode_device(parser, b["d"], b["o"], b["c"], b["rec"], None, b["flw"], b["lay"], stream=st)
        ev[1].record()
        groups = b["g"].group(b["d"], b["o"], b["c"], b["rec"], b["lay"], kind=flows.DEFRAG6, stream=st)
        ev[2].record()
        out = df6.defrag(b["d"], b["o"], b["c"], b["rec"], b["lay"], groups, out_data=out_data, data_cap=cap, stream=st)
        ev[3].record()
        return groups, out

    # re-emission: the batch's size does not bound the need; a first call says what it is
    probe = torch.empty(16, dtype=torch.uint8, device="cuda")
    _, out = one6(probe, 0)
    torch.cuda.synchronize()
    need = int(out["counts"][2].item())
    out6 = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    groups, out = one6(out6, need)
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    assert counts[3] == 0 and counts[2] == need
    move_bytes = need

    # IPv4: decoded and grouped once, its defrag (for its copy_kernel) in every run
    ctx.decode_device(parser, b4["d"], b4["o"], b4["c"], b4["rec"], None, b4["flw"], b4["lay"], stream=st)
    groups4 = b4["g"].group(b4["d"], b4["o"], b4["c"], b4["rec"], b4["lay"], kind=flows.DEFRAG, stream=st)
    out4 = torch.empty(b4["d"].numel() + 16, dtype=torch.uint8, device="cuda")

    def copy4():
        return df4.defrag(b4["d"], b4["o"], b4["c"], b4["rec"], b4["lay"], groups4, out_data=out4,
                          data_cap=b4["d"].numel(), stream=st)

    counts4 = copy4()["counts"].cpu().tolist()
    keyed = torch.nonzero(groups["group_of"] >= 0).flatten().to(torch.int32)
    keyed_bytes = int(b6["c"].index_select(0, keyed.long()).sum(dtype=torch.int64).item())
    src_len = min(move_bytes, b6["d"].numel())
    mc_src, mc_dst = b6["d"][:src_len], torch.empty(src_len, dtype=torch.uint8, device="cuda")

    def pack():
        return flows.pack_batch(b6["d"], b6["o"], b6["c"], keyed, total_bytes=keyed_bytes, stream=st)

    for _ in range(a.warmup):
        one6(out6, need)
        copy4()
        pack()
        mc_dst.copy_(mc_src)
    torch.cuda.synchronize()
    t = dict(decode=[], group=[], defrag=[], end_to_end=[], memcpy=[])
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(a.runs):  # the movers interleaved, so drift hits all alike
            one6(out6, need)
            copy4()
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

    plan = per_run("prep6_kernel", "plan6_kernel")
    move = per_run("move6_kernel")
    copy = per_run("copy_kernel")
    packk = per_run("pack_bytes_kernel")
    fin = per_run("finish6_kernel")
    props = torch.cuda.get_device_properties(0)
    res = dict(
        device=torch.cuda.get_device_name(0), arch=props.gcnArchName, compute_units=props.multi_processor_count,
        fragments=b6["n"], batch_bytes=int(b6["d"].numel()), datagrams=counts[0], pending=counts[1],
        groups=int(groups["counts"][0].item()), move_bytes=move_bytes, pack_bytes=keyed_bytes,
        ipv4=dict(fragments=b4["n"], batch_bytes=int(b4["d"].numel()), datagrams=counts4[0], copy_bytes=counts4[2]),
        method="one process, movers interleaved per run, %d timed runs after %d warm-up; stage times from events, "
               "kernel times from the profiler's device timeline; medians with min..max" % (a.runs, a.warmup),
        ms={k: spread(v) for k, v in t.items()},
    )
    if plan and move and copy and packk:
        scans = [x - p - q for x, p, q in zip(t["defrag"], plan, move)]
        res["ms"].update(plan=spread(plan), move=spread(move), scans_and_finish=spread(scans),
                         ipv4_copy_kernel=spread(copy), pack_bytes_kernel=spread(packk))
        if fin:
            res["ms"]["finish"] = spread(fin)
        mv = [move_bytes / (x * 1e6) for x in move]
        c4 = [counts4[2] / (x * 1e6) for x in copy]
        pk = [keyed_bytes / (x * 1e6) for x in packk]
        res["move_GBps"], res["ipv4_copy_GBps"], res["pack_GBps"] = spread(mv), spread(c4), spread(pk)
        res["move_over_ipv4_copy"] = spread([x / y for x, y in zip(mv, c4)])
        res["move_over_pack"] = spread([x / y for x, y in zip(mv, pk)])
    else:
        res["kernel_times"] = "the profiler returned no device timeline for the kernels"
        res["kernel_names_seen"] = sorted(kern)[:40]
    res["memcpy_GBps"] = spread([src_len / (x * 1e6) for x in t["memcpy"]])
    res["datagrams_per_s"] = counts[0] / (statistics.median(t["end_to_end"]) / 1e3)
    import reasm_time_ab
    seen = torch.arange(b6["n"], dtype=torch.int64, device="cuda") * 1000 + 1700000000 * 10 ** 9

    def call(**kw):
        return df6.defrag(b6["d"], b6["o"], b6["c"], b6["rec"], b6["lay"], groups, out_data=out6, data_cap=need,
                          stream=st, **kw)

    res["timed"] = reasm_time_ab.ab_rows(torch, profile, [ProfilerActivity.CPU, ProfilerActivity.CUDA], call,
                                         lambda: call(seen=seen), a.runs, a.warmup,
                                         shared=("prep6_kernel", "plan6_kernel"),
                                         timed_only=("key6_kernel", "drop6_kernel", "seen6_kernel"))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
