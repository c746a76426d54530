"""gpk_defrag_batch_timed and gpk_defrag6_batch_timed (LastSeen / the key's
time and DiscardOlderThan on the device, include/gpk_defrag.h,
include/gpk_defrag6.h) and the timed streaming classes of gopacket_amd.flows
against the timed model (tests/defrag_time_model.py) on the inputs whose
conditions tests/test_reasm_time_cpu.py checks: the same verdicts, datagrams,
pending list, key times and discard counts. No tolerance anywhere."""
import numpy as np
import pytest

import defrag6cases as D6
import defragcases as D4
import defragtimecases as TC
from configs import device_parser
from gopacket_amd import flows
from test_defrag6_gpu import device_decode as decode6
from test_defrag6_gpu import upload as upload6
from test_defrag_gpu import device_decode as decode4
from test_defrag_gpu import upload as upload4

pytestmark = pytest.mark.gpu

KEYS = ("last", "length", "payload_off", "offsets", "caplens")


def dev_seen(seen):
    import torch
    return torch.from_numpy(TC.as_int64(seen)).cuda()


def host(out, keys):
    counts = out["counts"].cpu().tolist()
    D, P = counts[0], counts[1]
    h = dict(verdict=out["verdict"].cpu().tolist(), counts=counts, pending=out["pending"][:P].cpu().tolist(),
             data=out["data"].cpu().numpy())
    for k in keys:
        h[k] = out[k][:D].cpu().tolist()
    if "pending_seen" in out:
        h["pending_seen"] = out["pending_seen"][:P].cpu().tolist()
        h["time_counts"] = out["time_counts"].cpu().tolist()
    return h


def device4(gpu_ctx, packets, seen=None, t=None):
    import torch
    _, (d, o, c) = upload4(packets)
    rec, lay = decode4(gpu_ctx, d, o, c)
    n = len(packets)
    g, df = flows.Grouper(max(n, 1)), flows.Defragmenter(max(n, 1))
    groups = g.group(d, o, c, rec, lay, kind=flows.DEFRAG)
    out = df.defrag(d, o, c, rec, lay, groups, seen=None if seen is None else dev_seen(seen), discard_older_than=t)
    torch.cuda.synchronize()
    h = host(out, KEYS)
    g.close()
    df.close()
    return h


def device6(gpu_ctx, packets, seen=None, t=None, carry=0, data_cap=None):
    import torch
    d, o, c = upload6(packets)
    rec, lay = decode6(gpu_ctx, d, o, c, TC.CFG6)
    n = len(packets)
    g, df = flows.Grouper(max(n, 1)), flows.Defragmenter6(max(n, 1))
    groups = g.group(d, o, c, rec, lay, kind=flows.DEFRAG6)
    out = df.defrag(d, o, c, rec, lay, groups, carry=carry, data_cap=data_cap,
                    seen=None if seen is None else dev_seen(seen), discard_older_than=t)
    torch.cuda.synchronize()
    h = host(out, KEYS + ("head",))
    g.close()
    df.close()
    return h


def compare(got, ref, discard, six=False):
    assert got["verdict"] == ref["verdict"]
    dg = ref["datagrams"]
    assert got["last"] == [d["last"] for d in dg]
    assert got["length"] == [d["length"] for d in dg]
    assert got["payload_off"] == [d["payload_off"] for d in dg]
    if six:
        assert got["head"] == [d["head"] for d in dg]
    for j, d in enumerate(dg):
        assert got["data"][got["offsets"][j]:got["offsets"][j] + got["caplens"][j]].tobytes() == d["data"], j
    assert got["pending"] == ref["pending"]
    assert got["pending_seen"] == ref["pending_seen"]
    assert got["counts"] == [len(dg), len(ref["pending"]), sum(len(d["data"]) for d in dg), 0]
    assert got["time_counts"] == (list(ref["discards"][0]) if discard else [0, 0])


def test_ipv4_conditions(gpu_ctx):
    pk, seen, t, pending, dropped = TC.conditions4()
    got = device4(gpu_ctx, pk, seen, t)
    compare(got, TC.model4(pk, seen, [(len(pk), t)]), True)
    assert got["pending"] == pending and got["time_counts"] == list(dropped)
    compare(device4(gpu_ctx, pk, seen), TC.model4(pk, seen), False)            # the key times without a discard
    for t2 in (t + 1, t - 1, TC.ts(0), TC.ts(1000)):                              # around the boundary, nothing, all
        compare(device4(gpu_ctx, pk, seen, t2), TC.model4(pk, seen, [(len(pk), t2)]), True)


def test_ipv6_conditions(gpu_ctx):
    pk, seen, t, pending, dropped = TC.conditions6()
    got = device6(gpu_ctx, pk, seen, t)
    compare(got, TC.model6(pk, seen, [(len(pk), t)]), True, six=True)
    assert got["pending"] == pending and got["time_counts"] == list(dropped)
    compare(device6(gpu_ctx, pk, seen), TC.model6(pk, seen), False, six=True)
    for t2 in (t + 1, t - 1, TC.ts(0), TC.ts(1000)):
        compare(device6(gpu_ctx, pk, seen, t2), TC.model6(pk, seen, [(len(pk), t2)]), True, six=True)
    # carried packets stamp too: with the first four as carry the times and the discard are the same
    ref = TC.model6(pk, seen, [(len(pk), t)], carry=4)
    compare(device6(gpu_ctx, pk, seen, t, carry=4), ref, True, six=True)
    assert ref["pending"] == pending


def test_discard_with_nothing_pending(gpu_ctx):
    rng = np.random.default_rng(3)
    pk = D4.fragments(1, D4.body(rng, 700), per=256) + [b"\x00" * 9]
    seen = [TC.ts(i) for i in range(len(pk))]
    got = device4(gpu_ctx, pk, seen, TC.ts(1000))
    compare(got, TC.model4(pk, seen, [(len(pk), TC.ts(1000))]), True)
    assert got["pending"] == [] and got["time_counts"] == [0, 0] and got["counts"][0] == 1
    pk = [b"\x00" * 9, D4.frag(1, 0, 1, b"a" * 16)]  # an IPv4 fragment is no IPv6 key: nothing keyed at all
    got = device6(gpu_ctx, pk, seen[:2], TC.ts(1000))
    compare(got, TC.model6(pk, seen[:2], [(2, TC.ts(1000))]), True, six=True)
    assert got["pending"] == [] and got["time_counts"] == [0, 0]
    # the streaming classes, empty
    for cls in (flows.IPv4Defragmenter, flows.IPv6Defragmenter):
        s = cls(gpu_ctx, device_parser(TC.CFG6), 16, timed=True)
        assert s.discard_older_than(TC.ts(5)) == 0
        with pytest.raises(ValueError):
            s.defrag(*upload6([pk[1]]))
        s.close()
        u = cls(gpu_ctx, device_parser(TC.CFG6), 16)
        with pytest.raises(NotImplementedError, match="out of scope"):
            u.discard_older_than(0)
        with pytest.raises(ValueError):
            u.defrag(*upload6([pk[1]]), dev_seen(seen[:1]))
        u.close()


def test_keys_wider_than_a_wave_and_many_keys(gpu_ctx):
    """Key times and discards where the plan kernels take their other paths: a
    key of 130 fragments (the large-list instantiation), and 700 keys (several
    blocks of the per-key kernel, wave-partial counts)."""
    rng = np.random.default_rng(9)
    big = [D4.frag(5, j, 1, D4.body(rng, 8)) for j in range(130)]
    many = [D4.frag(1000 + q, 0, 1, D4.body(rng, 8)) for q in range(700)]
    pk = many[:350] + big + many[350:]
    seen = [TC.ts(int(x)) for x in rng.integers(0, 100, len(pk))]
    t = TC.ts(50)
    ref = TC.model4(pk, seen, [(len(pk), t)])
    assert 200 < ref["discards"][0][0] < 500
    compare(device4(gpu_ctx, pk, seen, t), ref, True)
    big6 = [D6.frag6(5, j, 1, D6.body(rng, 8)) for j in range(130)]
    many6 = [D6.frag6(1000 + q, 1, 1, D6.body(rng, 8)) for q in range(700)]
    pk = many6[:350] + big6 + many6[350:] + [big6[7]]  # the big key's last call: a late duplicate
    seen = [TC.ts(int(x)) for x in rng.integers(0, 100, len(pk) - 1)] + [TC.ts(50)]
    ref = TC.model6(pk, seen, [(len(pk), t)])
    assert 200 < ref["discards"][0][0] < 500 and 350 in ref["pending"]
    compare(device6(gpu_ctx, pk, seen, t), ref, True, six=True)


def test_untimed_calls_unchanged(gpu_ctx):
    """gpk_defrag_batch and gpk_defrag_batch_timed without a discard give the
    same outputs on random traffic; the same for IPv6."""
    for six, pk in ((False, D4.random_traffic(4, 300, lo=2500, hi=7000, per=744)),
                    (True, D6.random_traffic(4, 300, lo=2500, hi=7000, per=744))):
        seen = [TC.ts(i) for i in range(len(pk))]
        if six:
            need = device6(gpu_ctx, pk)["counts"][2]
            a, b = device6(gpu_ctx, pk, data_cap=need), device6(gpu_ctx, pk, seen, data_cap=need)
        else:
            a, b = device4(gpu_ctx, pk), device4(gpu_ctx, pk, seen)
        assert a["counts"][0] > 100 and a["counts"][1] > 0 and a["counts"][3] == 0
        for k in ("verdict", "counts", "pending") + KEYS + (("head",) if six else ()):
            assert a[k] == b[k], k
        used = a["counts"][2]
        assert np.array_equal(a["data"][:used], b["data"][:used])
        assert b["time_counts"] == [0, 0] and len(b["pending_seen"]) == a["counts"][1]


def stream(gpu_ctx, cls, cfg, upload, pk, seen, ops, cut, **kw):
    """One run of the stream through a timed streaming class, cut into batches at
    the discards and at `cut` -> (verdicts, [(last, bytes)], discards, pending_seen)."""
    import torch
    s = cls(gpu_ctx, device_parser(cfg), 256, timed=True, **kw)
    verdicts, dgrams, discards = [], [], []
    for lo, hi, ts in TC.segments(len(pk), ops, cut):
        d, o, c = upload(pk[lo:hi])
        out = s.defrag(d, o[:hi - lo], c[:hi - lo], dev_seen(seen[lo:hi]))
        torch.cuda.synchronize()
        blob = out["data"].cpu().numpy()
        base = len(dgrams)
        for j in range(out["datagrams"]):
            at, ln = int(out["offsets"][j]), int(out["caplens"][j])
            dgrams.append((lo + int(out["last"][j]), blob[at:at + ln].tobytes()))
        verdicts += [v if v < 0 else v + base for v in out["verdict"].cpu().tolist()]
        discards += [s.discard_older_than(t) for t in ts]
    left = [] if s._pending_seen is None else sorted(s._pending_seen.cpu().tolist())
    assert len(left) == s.pending_count
    s.close()
    return verdicts, dgrams, discards, left


@pytest.mark.parametrize("six", [False, True], ids=["ipv4", "ipv6"])
def test_streaming_every_cut(gpu_ctx, six):
    """The ~60-fragment stream with three discards, cut into batches at every
    position: each run equals the model's single sequential run. For IPv6 the
    cuts between positions 37 and 41 carry key 900 with an ignored duplicate as
    its last stamper."""
    pk, seen, ops = TC.stream6() if six else TC.stream4()
    ref = (TC.model6 if six else TC.model4)(pk, seen, ops)
    want = (ref["verdict"], [(d["last"], d["data"]) for d in ref["datagrams"]], [k for k, _ in ref["discards"]],
            sorted(ref["pending_seen"]))
    cls, cfg, up = ((flows.IPv6Defragmenter, TC.CFG6, upload6) if six else
                    (flows.IPv4Defragmenter, TC.CFG4, lambda p: upload4(p)[1]))
    for cut in range(len(pk) + 1):
        got = stream(gpu_ctx, cls, cfg, up, pk, seen, ops, cut)
        for a, b, what in zip(got, want, ("verdict", "datagrams", "discards", "pending_seen")):
            assert a == b, (cut, what)
