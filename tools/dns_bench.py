#!/usr/bin/env python3
"""Measure gpk_dns_batch (include/gpk_dns.h) on one GPU.

Batches of --packets packets (default 1 Mi):
  imix_1_in_64   C4 (IMIX) generated in HBM (gopacket_amd.synth), every 64th
                 packet behind Ethernet / IPv4 / UDP port 53 and a DNS query
                 (the packet becomes trailing bytes, which DecodeFromBytes
                 ignores), as tools/control_bench.py puts an ICMP header there:
                 the pass where DNS is rare. Run tools/control_bench.py in the
                 same session for the comparison: boxes differ by several percent.
  queries        every packet one A query for a three-label name
  responses      every packet a response with a question, a CNAME and two A
                 answers, an NS authority and an OPT additional, names
                 compressed with pointers
and one batch of --adversarial (default 1 Ki) 1500-byte messages each:
  loop_255       a question name of 126 one-byte labels ending in a pointer to
                 its own start: 255 levels x 126 labels = 32 130 label steps in
                 one lane, then "max DNS recursion level hit". The bound per
                 name is 255 levels x 128 labels (a level holds at most 255
                 bytes, a label takes at least two, a pointer two more).
  long_names     the longest names that decode: five runs of 126 labels chained
                 by pointers inside a NULL record's RDATA, then as many records
                 as fit whose owner name is a pointer to the first run. Every
                 name is walked and written out again.
Per batch, median (min..max) over --runs timed runs after --warmup: the whole
call between two events, and its kernels from the profiler's device timeline
(classify, scatter, the two scans, emit), in ms and messages/s. The emit
shape is one lane per message.

  python tools/dns_bench.py --out profiles/dns.json
"""
import argparse
import json
import os
import re
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OWN = r"\b%s_kernel<.*DnsPass>"  # this pass's instantiation of a kernel template of csrc/gpk_postpass.h
MAC = bytes(range(1, 13))


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


def name(*labels, ptr=None):
    out = b"".join(bytes([len(x)]) + x for x in labels)
    return out + (struct.pack(">H", 0xc000 | ptr) if ptr is not None else b"\x00")


def rr(owner, typ, rdata=b"", cls=1, ttl=300):
    return owner + struct.pack(">HHIH", typ, cls, ttl, len(rdata)) + rdata


def frame(msg):
    udp = struct.pack(">HHHH", 50004, 53, 8 + len(msg), 0) + msg
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(udp), 1, 0, 64, 17, 0) + bytes([10, 0, 0, 1, 10, 0, 0, 2]) + udp
    return MAC + b"\x08\x00" + ip


QNAME = name(b"www", b"example", b"com")
QUERY = struct.pack(">HHHHHH", 0x1234, 0x0100, 1, 0, 0, 0) + QNAME + struct.pack(">HH", 1, 1)


def response():
    p = name(ptr=12)
    return (struct.pack(">HHHHHH", 0x1234, 0x8180, 1, 3, 1, 1) + QNAME + struct.pack(">HH", 1, 1) +
            rr(p, 5, name(b"edge", b"cdn", ptr=16)) + rr(name(ptr=45), 1, bytes([192, 0, 2, 1])) +
            rr(name(ptr=45), 1, bytes([192, 0, 2, 2])) + rr(name(ptr=16), 2, name(b"ns1", ptr=16)) +
            rr(b"\x00", 41, b"", cls=1232, ttl=0))


def loop_255(size=1500 - 42):
    msg = struct.pack(">HHHHHH", 1, 0x0100, 1, 0, 0, 0) + b"\x01a" * 126 + name(ptr=12) + struct.pack(">HH", 1, 1)
    return msg + bytes(size - len(msg)), 255 * 126


def long_names(size=1500 - 42):
    """(message, label steps of the walk in one mode)."""
    runs, per = 5, 126
    start = 12 + 1 + 10  # the NULL record's RDATA: behind the header, a root owner and the fixed fields
    blocks = b""
    for k in range(runs):
        nxt = start + (k + 1) * (2 * per + 2)
        blocks += b"\x01a" * per + (name(ptr=nxt) if k + 1 < runs else b"\x01z\x00")
    first = rr(b"\x00", 10, blocks)
    room = size - 12 - len(first)
    more = room // 12
    msg = struct.pack(">HHHHHH", 1, 0x8180, 0, 1 + more, 0, 0) + first + rr(name(ptr=start), 1, b"") * more
    return msg + bytes(size - len(msg)), more * (runs * per + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--adversarial", type=int, default=1 << 10)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile

    from gopacket_amd import _lib, engine, flows, synth

    n = a.packets
    prop = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               emit_shape="one lane per message",
               method="one process, %d timed runs after %d warm-up; call times between events, kernel times from the "
                      "profiler's device timeline; medians with min..max" % (a.runs, a.warmup), rows=[])
    ctx = engine.Context(0)
    kinds = [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP,
             _lib.DEC_PAYLOAD]
    parser = engine.ParserConfig(17, kinds)

    def encapsulate(d, o, c, header, len_at, every):
        """tools/control_bench.py's: header in front of every `every`-th packet, its length fields set."""
        m = o.numel()
        hl = len(header)
        h = torch.tensor(list(header), dtype=torch.uint8, device="cuda").repeat(m, 1)
        for at, k in len_at:
            v = c + k
            h[:, at] = (v >> 8).to(torch.uint8)
            h[:, at + 1] = (v & 255).to(torch.uint8)
        sel = (torch.arange(m, device="cuda") % every) == 0
        cat = torch.cat([h.flatten(), d])
        po = torch.stack([torch.arange(m, device="cuda", dtype=torch.int64) * hl, o + m * hl], 1).flatten()
        pc = torch.stack([torch.where(sel, hl, 0).int(), c], 1).flatten()
        od, oo, oc = flows.pack_batch(cat, po, pc, torch.arange(2 * m, device="cuda", dtype=torch.int32))
        pad = torch.zeros((od.numel() + 15) // 16 * 16 + 32, dtype=torch.uint8, device="cuda")
        pad[:od.numel()] = od
        return pad, oo[0::2].contiguous(), (oc[0::2] + oc[1::2]).contiguous()

    def tiled(pkt, count):
        stride = (len(pkt) + 15) // 16 * 16
        row = np.zeros(stride, np.uint8)
        row[:len(pkt)] = np.frombuffer(pkt, np.uint8)
        d = torch.from_numpy(np.concatenate([np.tile(row, count), np.zeros(32, np.uint8)])).cuda()
        o = torch.arange(count, dtype=torch.int64, device="cuda") * stride
        c = torch.full((count,), len(pkt), dtype=torch.int32, device="cuda")
        return d, o, c

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    def measure(label, d, o, c, extra):
        m = o.numel()
        rec = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
        err = torch.zeros(2 * m, dtype=torch.int32, device="cuda")
        fl = torch.zeros(3 * m, dtype=torch.int64, device="cuda")
        lay = torch.zeros(m * 64, dtype=torch.uint8, device="cuda")
        ctx.decode_device(parser, d, o, c, rec, err, fl, lay)
        dnd = flows.DNSDecoder(m)
        out = dnd.decode_all(ctx, d, o, c, rec, lay, parser)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().numpy().view(np.uint32)
        need_rr, need_nb = flows.DNSDecoder.needed(counts)

        def call():
            dnd.decode(ctx, d, o, c, rec, lay, parser, need_rr, need_nb, out=out)

        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ev = []
        for _ in range(a.runs):
            ev.append(timed(call))
            torch.cuda.synchronize()
        t = [x.elapsed_time(y) for x, y in ev]
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(a.runs):
                call()
                torch.cuda.synchronize()
        kern = kernel_times(prof)
        msgs = int(counts[0])
        emit = per_run(kern, a.runs, r"\bemit_kernel")
        row = dict(batch=label, packets=m, candidates=msgs, ok=int(counts[1]), failed=int(counts[2]), entries=need_rr,
                   name_bytes=need_nb, batch_bytes=int(c.sum(dtype=torch.int64).item()), pass_ms=spread(t),
                   messages_per_s=spread([msgs / (x * 1e-3) for x in t]) if msgs else None,
                   kernels_ms=dict(classify=per_run(kern, a.runs, OWN % "classify"),
                                   scatter=per_run(kern, a.runs, OWN % "scatter"),
                                   scan=per_run(kern, a.runs, "scan", "Scan", r"\bfinish_kernel<%d>" % _lib.DNS_NCLASS),
                                   emit=emit),
                   emit_messages_per_s=spread([msgs / (emit[k] * 1e-3) for k in ("median", "min", "max")])
                   if emit and msgs else None, **extra)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        dnd.close()

    hdr = frame(QUERY)
    d0, o0, c0 = synth.device_batch(synth.C4_IMIX, 0, n)
    d, o, c = encapsulate(d0, o0, c0, hdr, [(16, len(hdr) - 14), (38, len(hdr) - 34)], 64)
    del d0
    measure("imix_1_in_64", d, o, c, dict(source=synth.NAMES[synth.C4_IMIX], dns_one_in=64))
    del d, o, c
    measure("queries", *tiled(frame(QUERY), n), dict(message_bytes=len(QUERY)))
    measure("responses", *tiled(frame(response()), n), dict(message_bytes=len(response())))
    for label, (msg, steps) in (("loop_255", loop_255()), ("long_names", long_names())):
        measure(label, *tiled(frame(msg), a.adversarial),
                dict(message_bytes=len(msg), label_steps_per_message=steps,
                     bound_per_name="255 levels x 128 labels"))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
