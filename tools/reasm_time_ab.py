"""The timed row of tools/tcpasm_bench.py, tools/defrag_bench.py and
tools/defrag6_bench.py: the same batch through the untimed and the timed entry
point of a reassembler (include/gpk_tcpasm.h, gpk_defrag.h, gpk_defrag6.h),
interleaved run by run in one process, so that drift hits both alike.

Per run the untimed call goes first, then the timed one; each is timed with
stream events, and the profiler's device timeline gives the plan kernels of
each (prep + plan, and for the timed call the kernels time adds). Kernels both
calls launch under one name are told apart by launch order inside a run.
"""
import statistics


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def _has(name, pieces):
    return any(p in name for p in pieces)


def ab_rows(torch, profile, activities, untimed, timed, runs, warmup, shared, untimed_only=(), timed_only=()):
    """untimed(), timed(): launch one reassembly call each on the current stream.
    shared: name pieces of the plan kernels both launch; untimed_only /
    timed_only: pieces of the plan kernels only one of them launches.
    -> dict(ms: call and plan of both, min..max; ratios of the medians)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(warmup):
        untimed()
        timed()
    torch.cuda.synchronize()
    ta, tb = [], []
    with profile(activities=activities) as prof:
        for _ in range(runs):
            ev[0].record()
            untimed()
            ev[1].record()
            timed()
            ev[2].record()
            torch.cuda.synchronize()
            ta.append(ev[0].elapsed_time(ev[1]))
            tb.append(ev[1].elapsed_time(ev[2]))
    kern = {}
    for e in prof.events():
        if "cuda" not in str(getattr(e, "device_type", "")).lower():
            continue
        us = getattr(e, "device_time", None)
        if us is None:
            us = getattr(e, "cuda_time", 0.0)
        kern.setdefault(e.name, []).append(us / 1000.0)
    pa, pb, added = [0.0] * runs, [0.0] * runs, [0.0] * runs
    seen_any = False
    for name, xs in kern.items():
        if not xs or len(xs) % runs:
            continue
        k = len(xs) // runs
        per = [xs[i * k:(i + 1) * k] for i in range(runs)]
        if _has(name, timed_only):
            for i, p in enumerate(per):
                pb[i] += sum(p)
                added[i] += sum(p)
            seen_any = True
        elif _has(name, untimed_only):
            for i, p in enumerate(per):
                pa[i] += sum(p)
            seen_any = True
        elif _has(name, shared) and k % 2 == 0:
            for i, p in enumerate(per):
                pa[i] += sum(p[:k // 2])
                pb[i] += sum(p[k // 2:])
            seen_any = True
    res = dict(method="untimed then timed call per run, %d runs after %d warm-ups, one process; call times from stream "
                      "events, plan (prep + plan kernels, plus what time adds) from the profiler's device timeline"
                      % (runs, warmup),
               ms=dict(untimed_call=spread(ta), timed_call=spread(tb)),
               call_ratio=statistics.median(tb) / statistics.median(ta))
    if seen_any and min(pa) > 0:
        res["ms"].update(untimed_plan=spread(pa), timed_plan=spread(pb), timed_only_kernels=spread(added))
        res["plan_ratio"] = statistics.median(pb) / statistics.median(pa)
    else:
        res["kernel_times"] = "the profiler returned no device timeline for the kernels"
        res["kernel_names_seen"] = sorted(kern)[:40]
    return res
