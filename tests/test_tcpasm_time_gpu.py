"""gpk_tcpasm_batch_timed (lastSeen, page.Seen and FlushWithOptions{T} on the
device, include/gpk_tcpasm.h), the timed flows.TCPAssembler and the timed
tcpassembly mirror against the timed model (tests/tcpasm_time_model.py) on the
inputs whose conditions tests/test_reasm_time_cpu.py checks: every array of
gpk_tcpasm_batch's comparison, plus lastSeen per connection and the flushed and
closed counts. No tolerance anywhere."""
import numpy as np
import pytest

import pktutil
import tcpasm_model as M
import tcpasmcases as TC
import tcpasmtimecases as TT
from configs import device_parser
from gopacket_amd import _lib, flows
from oracle import flows_oracle as FO
from test_tcpasm_gpu import compare, upload

pytestmark = pytest.mark.gpu
CFG = TT.CFG


def dev_seen(seen):
    import torch
    return torch.from_numpy(TT.as_int64(seen)).cuda()


def device_assemble(gpu_ctx, packets, seen=None, mode=0, t=0, max_pages=0, flush=False):
    """test_tcpasm_gpu.device_assemble with time -> host dict, plus conn_last_seen and time_counts"""
    import torch
    d, o, c = upload(packets)
    m = max(len(packets), 1)
    rec = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(3 * m, dtype=torch.int64, device="cuda")
    lay = torch.zeros(m * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(device_parser(CFG), d, o, c, rec, None, fl, lay, stream=torch.cuda.current_stream())
    g, asm = flows.Grouper(m), flows.Assembler(m)
    groups = g.group(d, o, c, rec, lay, kind=FO.CONNECTION)
    kw = {} if seen is None else dict(seen=dev_seen(seen), flush_older=mode, t=t)
    out = asm.assemble(d, o, c, rec, lay, groups, max_pages=max_pages, flush=flush, **kw)
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    G = int(groups["counts"][0].item())
    St = counts[0]
    host = dict(counts=counts, G=G, verdict=out["verdict"].cpu().tolist(), stream_of=out["stream_of"].cpu().tolist(),
                data=out["data"].cpu().numpy(), chunks=out["chunks"].cpu().numpy().view(_lib.TCP_CHUNK_DTYPE),
                stream_group=out["stream_group"][:St].cpu().tolist(), stream_first=out["stream_first"][:St].cpu().tolist(),
                stream_closed=out["stream_closed"][:St].cpu().numpy().view(np.uint32).tolist(),
                stream_chunk0=out["stream_chunk0"][:St + 1].cpu().tolist(),
                stream_data0=out["stream_data0"][:St + 1].cpu().tolist(),
                conn_seq=out["conn_seq"][:G].cpu().tolist(), conn_stream=out["conn_stream"][:G].cpu().tolist(),
                pend_pkt=out["pend_pkt"].cpu().tolist(), pend_page=out["pend_page"].cpu().tolist())
    if seen is not None:
        host["conn_last_seen"] = out["conn_last_seen"][:G].cpu().tolist()
        host["time_counts"] = out["time_counts"].cpu().tolist()
    g.close()
    asm.close()
    return host


def check(gpu_ctx, packets, seen, mode=0, t=0, max_pages=0):
    ops = [(len(packets), t, mode == 2)] if mode else []
    ref = TT.device_codes(TT.model(packets, seen, ops, max_pages=max_pages))
    got = device_assemble(gpu_ctx, packets, seen, mode, t, max_pages)
    compare(got, ref)
    assert got["conn_last_seen"] == ref["conn_last_seen"]
    assert got["time_counts"] == (list(ref["flushes"][0]) if mode else [0, 0])
    return ref, got


def test_last_seen_across_the_wave_step(gpu_ctx):
    pk, seen, want = TT.last_seen_keys()
    ref, got = check(gpu_ctx, pk, seen)
    assert got["conn_last_seen"] == want
    # CloseAll on lastSeen: T == lastSeen keeps the connection, one nanosecond more closes it
    for q in (0, 3, len(want) - 2):
        for t in (want[q], want[q] + 1):
            ref, got = check(gpu_ctx, pk, seen, 2, t)
            assert (got["conn_seq"][q] == M.NO_CONN) == (t > want[q])


@pytest.mark.parametrize("max_pages", [0, 2])
def test_boundaries(gpu_ctx, max_pages):
    pk, seen, names = TT.boundary_keys()
    T = TT.ts(TT.EDGE)
    for mode in (2, 1):
        ref, got = check(gpu_ctx, pk, seen, mode, T, max_pages)
        if not max_pages:
            assert got["time_counts"] == ([7, 4] if mode == 2 else [6, 1])
    check(gpu_ctx, pk, seen, 2, T + 1, max_pages)          # first==T goes too
    check(gpu_ctx, pk, seen, 2, TT.ts(0), max_pages)       # nothing is old
    check(gpu_ctx, pk, seen, 2, TT.ts(10 ** 6), max_pages)  # everything is
    check(gpu_ctx, pk, seen, 0, 0, max_pages)


def test_long_list_past_lds(gpu_ctx):
    pk, seen, T = TT.long_list()
    ref, got = check(gpu_ctx, pk, seen, 2, T)
    assert got["counts"][1] == 270 and got["counts"][3] == 30 and got["time_counts"] == [1, 0]
    check(gpu_ctx, pk, seen, 2, TT.ts(1000))  # all 300 rounds, then CloseAll


def test_untimed_call_unchanged(gpu_ctx):
    """gpk_tcpasm_batch and gpk_tcpasm_batch_timed with flush_older = 0 give
    identical outputs on random traffic, with and without FlushAll; and flush
    together with flush_older is an argument error."""
    pk = TC.random_traffic(7, 600)
    seen = [TT.ts(i) for i in range(len(pk))]
    for flush in (False, True):
        for mp in (0, 4):
            a = device_assemble(gpu_ctx, pk, None, max_pages=mp, flush=flush)
            b = device_assemble(gpu_ctx, pk, seen, max_pages=mp, flush=flush)
            assert a["counts"][0] > 600
            C, D, NP = a["counts"][1], a["counts"][2], a["counts"][3]
            for k in a:
                if k == "chunks":
                    assert a[k][:C].tobytes() == b[k][:C].tobytes()
                elif k == "data":
                    assert np.array_equal(a[k][:D], b[k][:D])
                elif k in ("pend_pkt", "pend_page"):
                    assert a[k][:NP] == b[k][:NP]
                else:
                    assert a[k] == b[k], k
            assert b["time_counts"] == [0, 0]
    with pytest.raises(_lib.GpkError):
        device_assemble(gpu_ctx, pk[:10], seen[:10], mode=2, t=5, flush=True)


def stream_key(s):
    return [(c["src"], c["src_off"], c["len"], c["skip"], c["flags"], c["call"], c["seen"]) for c in s["chunks"]]


def run_streaming(gpu_ctx, pk, seen, ops, cut, max_pages=0):
    """-> ({global stream id: (chunk tuples with global src and call, bytes, closing call)}, [(flushed, closed)],
    the open set: sorted (stream id, lastSeen, pages))"""
    s = flows.TCPAssembler(gpu_ctx, device_parser(CFG), 256, max_pages=max_pages, timed=True)
    acc, flushes, starts = {}, [], []

    def take(res, op):
        def call(c):
            return ("flush", op, c[1]) if c[0] == "flush" else starts[c[0]] + c[1]
        blob = res["data"].cpu().numpy() if res["streams"] else None
        for st in res["streams"]:
            e = acc.setdefault(st["id"], [[], [], M.OPEN])
            for ch in st["chunks"]:
                b, i = ch["src"]
                e[0].append((starts[b] + i, ch["src_off"], ch["len"], ch["skip"], ch["flags"], call(ch["call"]),
                             ch["seen"]))
            e[1].append(blob[st["data0"]:st["data1"]].tobytes())
            if st["closed"] is not None:
                e[2] = call(st["closed"])

    for lo, hi, after in TT.segments(len(pk), ops, cut):
        starts.append(lo)
        d, o, c = upload(pk[lo:hi])
        take(s.assemble(d, o, c, dev_seen(seen[lo:hi])), None)
        for k in after:
            res = s.flush_older_than(ops[k][1], close_all=ops[k][2])
            take(res, k)
            flushes.append((res["flushed"], res["closed"]))
    left = []
    if s._carry is not None:
        code, gid = s._carry[3], s._carry[5]
        for j, cd in enumerate(code):
            if cd & _lib.TCPASM_CARRY_CONN:
                left.append([gid[j], s._carry_seen[j], []])
            else:
                left[-1][2].append(s._carry_seen[j])
    assert s.open_count == len(left)
    s.close()
    return ({k: (v[0], b"".join(v[1]), v[2]) for k, v in acc.items()}, flushes,
            sorted((sid, last, tuple(pages)) for sid, last, pages in left))


def stream_reference(pk, seen, ops, max_pages=0):
    ref = TT.model(pk, seen, ops, max_pages=max_pages)
    want = {j: (stream_key(s), s["data"], s["closed"]) for j, s in enumerate(ref["streams"])}
    left = []
    pages = {}
    for (p, _), sn in zip(ref["pend"], ref["pend_seen"]):
        pages.setdefault(ref["stream_of"][p], []).append(sn)
    for g, j in enumerate(ref["conn_stream"]):
        if j >= 0:
            left.append((j, ref["conn_last_seen"][g], tuple(pages.get(j, ()))))
    return ref, want, ref["flushes"], sorted(left)


def test_streaming_every_cut(gpu_ctx):
    """The 150-packet sequence with its three flushes, cut into batches at every
    position: each run equals the model's single sequential run on the chunks
    (source, Skip, flags, call, Seen), the bytes, the closing calls, flushed and
    closed per flush, and the final open set with lastSeen and the pages' Seen."""
    pk, seen, ops = TT.stream()
    _, want, flushes, left = stream_reference(pk, seen, ops)
    for cut in range(len(pk) + 1):
        got = run_streaming(gpu_ctx, pk, seen, ops, cut)
        assert got[1] == flushes, cut
        assert got[0] == want, cut
        assert got[2] == left, cut
    _, want, flushes, left = stream_reference(pk, seen, ops, max_pages=2)
    for cut in range(0, len(pk) + 1, 9):
        assert run_streaming(gpu_ctx, pk, seen, ops, cut, max_pages=2) == (want, flushes, left), cut


def test_host_mirror_with_flush_older_than(gpu_ctx):
    """The timed tcpassembly mirror over the same sequence: the model's call
    log, New / Reassembled (with Seen) / ReassemblyComplete, in the same order,
    and (flushed, closed) from every FlushWithOptions."""
    from gopacket_amd import tcpassembly
    pk, seen, ops = TT.stream()
    ref = TT.model(pk, seen, ops)
    want, idx = [], {}
    for e in ref["log"]:
        if e[0] == "Reassembled":
            st = ref["streams"][e[1]]
            k = idx.get(e[1], 0)
            idx[e[1]] = k + e[3]
            at = sum(c["len"] for c in st["chunks"][:k])
            items = []
            for c in st["chunks"][k:k + e[3]]:
                items.append((st["data"][at:at + c["len"]], c["skip"], bool(c["flags"] & M.START),
                              bool(c["flags"] & M.END), c["seen"]))
                at += c["len"]
            want.append(("Reassembled", e[1], items))
        else:
            want.append((e[0], e[1]))
    got = []

    class Stream(tcpassembly.Stream):
        def __init__(self, j):
            self.j = j

        def Reassembled(self, rs):
            got.append(("Reassembled", self.j, [(bytes(r.Bytes), r.Skip, r.Start, r.End, r.Seen) for r in rs]))

        def ReassemblyComplete(self):
            got.append(("ReassemblyComplete", self.j))

    class Factory(tcpassembly.StreamFactory):
        n = 0

        def New(self, net, transport):
            got.append(("New", Factory.n))
            Factory.n += 1
            return Stream(Factory.n - 1)

    a = tcpassembly.NewAssembler(tcpassembly.NewStreamPool(Factory()), ctx=gpu_ctx, parser=device_parser(CFG),
                                 max_packets=1024, timed=True)
    flushes = []
    for lo, hi, after in TT.segments(len(pk), ops, 77):
        data, off, cap = pktutil.pack(pk[lo:hi])
        ts = TT.as_int64(seen[lo:hi])
        if lo == 0:  # the capture-info form of the same timestamps
            ci = np.zeros(hi - lo, _lib.CAPINFO_DTYPE)
            ci["ts_sec"], ci["ts_nsec"] = ts // 10 ** 9, ts % 10 ** 9
            ts = ci
        a.AssembleBatch(data, off[:hi - lo], cap[:hi - lo], timestamps=ts)
        for k in after:
            if ops[k][2]:
                flushes.append(a.FlushOlderThan(ops[k][1]))
            else:
                flushes.append(a.FlushWithOptions(tcpassembly.FlushOptions(T=ops[k][1], CloseAll=False)))
    assert got == want
    assert flushes == ref["flushes"]
    with pytest.raises(ValueError):
        a.AssembleBatch(*pktutil.pack(pk[:2]))
    a.close()
    assert int(flows.timestamps_ns(ci)[3]) == seen[3]
