#!/usr/bin/env python3
"""Measure gpk_svc_batch (include/gpk_svc.h) on one GPU, beside gpk_ndp_batch on
its own benchmark frame (tools/ndp_bench.py's Neighbor Solicitation) in the
same process: the service pass is the NDP pass's shape, so that is its
yardstick.

Input: batches in HBM. The first three repeat one frame 1 Mi times (Ethernet /
IP / UDP / message); the fourth is IMIX (gopacket_amd.synth C4) with every 64th
packet replaced by the DHCPv4 frame; the last is the pass's worst case and is
measured in a 1 Ki-packet batch only:
  dhcp4_discover_8   DHCPv4 Discover with eight options and an End
  dhcp6_solicit_5    DHCPv6 Solicit with five options
  ntp_48             a 48-byte NTP client message
  imix_1_in_64       IMIX, every 64th packet the Discover
  dhcp4_300_pads     a DHCPv4 message of 300 Pad bytes: 300 entries per message
Per batch, median (min..max) over --runs timed runs after --warmup: the whole
gpk_svc_batch call between two events with the capacity the batch needs, the
sizing call with capacity 0, gpk_ndp_batch with exact capacity on 1 Mi of its
frame in the same loop, and the service call's kernels from the profiler's
device timeline (classify, the first scan with finish, scatter, the second
scan, emit).

  python tools/svc_bench.py --out profiles/svc.json
"""
import argparse
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ndp_bench import frames as ndp_frames, kernel_times, per_run, spread  # noqa: E402

OWN = r"\b%s_kernel<.*SvcPass>"  # this pass's instantiation of a kernel template of csrc/gpk_postpass.h


def frames():
    """The four frames, checksums not set (the pass does not look at them)."""
    mac = bytes(range(1, 13))

    def udp4(msg, sport, dport):
        u = struct.pack(">HHHH", sport, dport, 8 + len(msg), 0) + msg
        ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(u), 0, 0, 64, 17, 0) + bytes([10, 0, 0, 1]) + bytes([10, 0, 0, 2])
        return mac + b"\x08\x00" + ip + u

    def udp6(msg, sport, dport):
        u = struct.pack(">HHHH", sport, dport, 8 + len(msg), 0) + msg
        ip6 = struct.pack(">IHBB", 6 << 28, len(u), 17, 255) + bytes.fromhex("fe80" + "00" * 13 + "01") + \
            bytes.fromhex("ff02" + "00" * 11 + "010002")
        return mac + b"\x86\xdd" + ip6 + u

    def opt4(t, d):
        return bytes([t, len(d)]) + d

    def opt6(c, d):
        return struct.pack(">HH", c, len(d)) + d
    hw = bytes.fromhex("000c29a1b2c3")
    head = struct.pack(">BBBBIHH", 1, 1, 6, 0, 0x3903f326, 0, 0x8000) + bytes(16) + hw.ljust(16, b"\x00") + bytes(192) + \
        bytes.fromhex("63825363")
    discover = head + opt4(53, b"\x01") + opt4(61, b"\x01" + hw) + opt4(12, b"host-1") + opt4(60, b"MSFT 5.0") + \
        opt4(50, bytes([10, 0, 0, 99])) + opt4(55, bytes([1, 3, 6, 15, 31, 33, 43, 44, 46, 47, 121, 249, 252])) + \
        opt4(57, b"\x05\xdc") + opt4(51, struct.pack(">I", 3600)) + b"\xff"
    duid = bytes.fromhex("000100011c39cf88080027fe8f95")
    solicit = bytes.fromhex("011a2b3c") + opt6(1, duid) + opt6(6, b"\x00\x17\x00\x18") + opt6(8, b"\x00\x00") + opt6(14, b"") + \
        opt6(3, struct.pack(">III", 0x0027fe8f, 0, 0))
    ntp = struct.pack(">BBBBIII4Q", 0x23, 2, 6, 0xe9, 0xa8c, 0x123d, 0xc0a80001, 1, 2, 3, 4)
    return dict(dhcp4_discover_8=(udp4(discover, 68, 67), 8), dhcp6_solicit_5=(udp6(solicit, 546, 547), 5),
                ntp_48=(udp4(ntp, 50123, 123), 0), dhcp4_300_pads=(udp4(head + bytes(300), 68, 67), 300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--pad-packets", type=int, default=1 << 10)
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
                      "profiler's device timeline; medians with min..max; gpk_ndp_batch on %d of its own benchmark "
                      "frames in the same loop" % (a.runs, a.warmup, n), rows=[])
    ctx = engine.Context(0)
    kinds = [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP,
             _lib.DEC_PAYLOAD]
    parser = engine.ParserConfig(17, kinds)
    svd, ndd = flows.ServiceDecoder(n), flows.NDPDecoder(n)
    fr = frames()

    def outputs(count):
        return (torch.zeros(count * 16, dtype=torch.uint8, device="cuda"), torch.zeros(2 * count, dtype=torch.int32, device="cuda"),
                torch.zeros(3 * count, dtype=torch.int64, device="cuda"), torch.zeros(count * 64, dtype=torch.uint8, device="cuda"))

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

    # the yardstick: the NDP pass on its own frame, decoded once, timed in every batch's loop
    yd, yo, yc = repeated(ndp_frames()["ns_1_option"], n)
    yrec, yerr, yfl, ylay = outputs(n)
    ctx.decode_device(parser, yd, yo, yc, yrec, yerr, yfl, ylay)
    ysized = ndd.decode(ctx, yd, yo, yc, yrec, ylay, parser, 0)
    torch.cuda.synchronize()
    yneed = flows.NDPDecoder.needed(ysized["counts"].cpu().numpy().view("u4"))
    yout = ndd.decode(ctx, yd, yo, yc, yrec, ylay, parser, yneed)
    torch.cuda.synchronize()
    assert int(yout["counts"][0].item()) == n and yneed == n

    batches = [(name, lambda f=fr[name][0]: repeated(f, n), n, 1, fr[name][1])
               for name in ("dhcp4_discover_8", "dhcp6_solicit_5", "ntp_48")]
    batches.append(("imix_1_in_64", lambda: imix(fr["dhcp4_discover_8"][0], 64), n, 64, 8))
    batches.append(("dhcp4_300_pads", lambda: repeated(fr["dhcp4_300_pads"][0], a.pad_packets), a.pad_packets, 1, 300))
    for name, make, count, every, per in batches:
        d, o, c = make()
        rec, err, fl, lay = outputs(count)
        ctx.decode_device(parser, d, o, c, rec, err, fl, lay)
        sized = svd.decode(ctx, d, o, c, rec, lay, parser, 0)
        torch.cuda.synchronize()
        need = flows.ServiceDecoder.needed(sized["counts"].cpu().numpy().view("u4"))
        out = svd.decode(ctx, d, o, c, rec, lay, parser, need)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().numpy().view("u4").tolist()
        cand = (count + every - 1) // every
        assert not counts[3] and counts[2] == 0 and counts[0] == cand and need == cand * per, (counts, need)

        calls = dict(svc_ms=lambda: svd.decode(ctx, d, o, c, rec, lay, parser, need, out=out),
                     svc_sizing_ms=lambda: svd.decode(ctx, d, o, c, rec, lay, parser, 0, out=sized),
                     ndp_yardstick_ms=lambda: ndd.decode(ctx, yd, yo, yc, yrec, ylay, parser, yneed, out=yout))
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
                calls["svc_ms"]()
                torch.cuda.synchronize()
        kern = kernel_times(prof)
        scans = per_run(kern, a.runs, "scan", "Scan", r"\bfinish_kernel<%d>" % _lib.SVC_NCLASS)
        row = dict(batch=name, svc_one_in=every, packets=count, candidates=counts[0], entries=need,
                   batch_bytes=int(c.sum(dtype=torch.int64).item()), **t,
                   svc_messages_per_s=counts[0] / (t["svc_ms"]["median"] * 1e-3),
                   kernels_ms=dict(classify=per_run(kern, a.runs, OWN % "classify"),
                                   scatter=per_run(kern, a.runs, OWN % "scatter"), scans_and_finish=scans,
                                   emit=per_run(kern, a.runs, r"\bemit_kernel")))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del d, o, c, out, sized, rec, err, fl, lay
    svd.close()
    ndd.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
