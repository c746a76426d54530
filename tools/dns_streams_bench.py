#!/usr/bin/env python3
"""Measure gpk_dns_streams (include/gpk_dns_streams.h) on one GPU, beside the
gpk_tcpasm_batch call that feeds it, of the same run and the same packets.

Cases (sizes scale with --streams, default 64 Ki, --singles, default 1 Mi, and
--zone-messages, default 90 000):
  exchanges     --streams connections of a SYN and a 29-byte query and a
                six-entry response (A, AAAA, CNAME, MX, TXT, OPT) in segments
                of 80 bytes
  singles       --singles connections of a SYN and one response in two segments
  exchanges_x4  the first case again, fed in four calls (SYN and one segment,
                then a segment per call) through flows.DNSStreams: the pass with
                carried tails and seam messages. Only the pass is timed there
                (the same call repeated on the state it had); the wrapper's host
                work is not.
  zone          one connection that holds --zone-messages messages of 36 bytes
                in segments of 1448 bytes: the zone-transfer shape, one lane's
                chase and one lane per message for the decode
Per case, median (min..max) over --runs timed runs after --warmup, each call
between two events. streams_ms is the pass with capacities that hold
everything. sizing_ms is the same call with every capacity 0 (init, cut, one
chase per stream, the scan: nothing is placed), placed_ms the call with the
message and tail capacities only (both chases and the size walk: no entry or
name is written); their differences say where the time goes.

  python tools/dns_streams_bench.py --out profiles/dns_streams.json
"""
import argparse
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAC = bytes(range(1, 13))
MSS = 1448
CASES = ("exchanges", "singles", "exchanges_x4", "zone")


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs)) if xs else None


def name(*labels, ptr=None):
    out = b"".join(bytes([len(x)]) + x for x in labels)
    return out + (struct.pack(">H", 0xc000 | ptr) if ptr is not None else b"\x00")


def rr(nm, typ, rdata=b"", cls=1, ttl=300):
    return nm + struct.pack(">HHIH", typ, cls, ttl, len(rdata)) + rdata


QEX = name(b"example", b"com") + struct.pack(">HH", 1, 1)
P = name(ptr=12)


def pre(msg):
    return struct.pack(">H", len(msg)) + msg


def query(ident=0x1234):
    return struct.pack(">HHHHHH", ident, 0x0100, 1, 0, 0, 0) + QEX


def response(ident=0x1234):
    return (struct.pack(">HHHHHH", ident, 0x8180, 1, 5, 0, 1) + QEX + rr(P, 1, bytes([192, 0, 2, 1])) +
            rr(P, 28, bytes(range(16))) + rr(P, 5, name(b"www", ptr=12)) +
            rr(P, 15, struct.pack(">H", 10) + name(b"mail", ptr=12)) + rr(P, 16, b"\x03abc\x05hello") +
            rr(b"\x00", 41, struct.pack(">HH", 10, 8) + bytes(8), cls=4096, ttl=0))


def small(i):
    """A 36-byte message: one question whose first label tells the messages apart."""
    m = struct.pack(">HHHHHH", i & 0xFFFF, 0x8180, 1, 0, 0, 0) + name(b"m%07d" % (i % 10 ** 7), b"zone", b"test") + \
        struct.pack(">HH", 1, 1)
    assert len(m) == 36
    return m


def frame(payload, seq, flags=0x10):
    tcp = struct.pack(">HHIIBBHHH", 40000, 53, seq & 0xFFFFFFFF, 0, 0x50, flags, 1000, 0, 0) + payload
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(tcp), 1, 0, 64, 6, 0) + bytes([10, 0, 0, 1, 10, 0, 0, 2]) + tcp
    return MAC + b"\x08\x00" + ip


def connection(payload, seg):
    """SYN, then the payload in segments of `seg` bytes."""
    return [frame(b"", 1000, 0x02)] + [frame(payload[at:at + seg], 1001 + at) for at in range(0, len(payload), seg)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1 << 16)
    ap.add_argument("--singles", type=int, default=1 << 20)
    ap.add_argument("--zone-messages", type=int, default=90000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    from gopacket_amd import _lib, engine, flows

    D = flows.DNSStreamDecoder
    prop = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               shape="one lane per chunk for the cut, one lane per stream for the two chases over the length prefixes, "
                     "one lane per message for the size and the emit walk, a wave per tail",
               method="one process, %d timed runs after %d warm-up; each call between events; medians with min..max; "
                      "tcpasm_ms and the three timings of the pass are of the same run and the same packets" % (
                          a.runs, a.warmup),
               rows=[])
    ctx = engine.Context(0)
    parser = engine.ParserConfig(17, [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT,
                                      _lib.DEC_TCP, _lib.DEC_UDP, _lib.DEC_PAYLOAD])

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return t

    def tiled(frames, count):
        """`count` connections of `frames`, connection-major; connection k's source address is 10.k."""
        stride = (max(len(f) for f in frames) + 15) & ~15
        rows = np.zeros((len(frames), stride), np.uint8)
        for k, f in enumerate(frames):
            rows[k, :len(f)] = np.frombuffer(f, np.uint8)
        d = torch.from_numpy(rows).cuda().repeat(count, 1, 1)  # [count, frames, stride]
        ids = torch.arange(count, device="cuda", dtype=torch.int64)
        for b in range(3):
            d[:, :, 27 + b] = ((ids >> (16 - 8 * b)) & 255).to(torch.uint8)[:, None]
        caps = torch.tensor([len(f) for f in frames], dtype=torch.int32, device="cuda").repeat(count)
        offs = torch.arange(count * len(frames), dtype=torch.int64, device="cuda") * stride
        return torch.cat([d.flatten(), torch.zeros(32, dtype=torch.uint8, device="cuda")]), offs, caps

    def three(dec, args, need, carry=None, tails=None):
        """The pass with every capacity 0, with the stream level's only, and with all four."""
        out = dec.decode(*args, *need, carry=carry)
        if tails is not None:
            out["tails"] = tails
        torch.cuda.synchronize()
        t_all = timed(lambda: dec.decode(*args, *need, carry=carry, out=out))
        t_placed = timed(lambda: dec.decode(*args, need[0], 0, 0, need[3], carry=carry, out=out))
        t_sizing = timed(lambda: dec.decode(*args, 0, 0, 0, 0, carry=carry, out=out))
        dec.decode(*args, *need, carry=carry, out=out)  # leave the outputs whole
        torch.cuda.synchronize()
        return t_all, t_placed, t_sizing

    def one_call(label, d, o, c, extra):
        n = o.numel()
        grouper, asm = flows.Grouper(n), flows.Assembler(n)
        rec_, lay, groups, st = flows._decode_group(ctx, parser, grouper, d, o, c, flows.CONNECTION)
        ao = asm.assemble(d, o, c, rec_, lay, groups)
        t_asm = timed(lambda: asm.assemble(d, o, c, rec_, lay, groups, out_data=ao["data"], data_cap=d.numel()))
        args = (ctx, parser, d, o, c, rec_, lay, ao)
        sizing = D(n, 1)
        counts = sizing.decode(*args, 0, 0, 0, 0)["counts"].cpu().tolist()
        sizing.close()
        dec = D(n, max(counts[5], 1))
        out = dec.decode_all(*args)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().tolist()
        need = D.needed(counts)
        t_all, t_placed, t_sizing = three(dec, args, need)
        row = dict(case=label, packets=n, batch_bytes=int(c.sum(dtype=torch.int64).item()), streams=counts[0],
                   streams_framed=counts[1], messages=counts[2], failed_messages=counts[3], rr_entries=need[1],
                   name_bytes=need[2], tail_bytes=need[3], tcpasm_ms=spread(t_asm), streams_ms=spread(t_all),
                   placed_ms=spread(t_placed), sizing_ms=spread(t_sizing),
                   streams_over_tcpasm=statistics.median(t_all) / statistics.median(t_asm), **extra)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        for h in (grouper, asm, dec):
            h.close()

    def want(label):
        return a.only in (None, label)

    exchange = pre(query()) + pre(response())
    if want("exchanges"):
        frames = connection(exchange, 80)
        one_call("exchanges", *tiled(frames, a.streams),
                 dict(segments_per_stream=len(frames) - 1, stream_bytes=len(exchange), messages_per_stream=2))
    if want("singles"):
        one = pre(response())
        frames = connection(one, (len(one) + 1) // 2)
        assert len(frames) == 3
        one_call("singles", *tiled(frames, a.singles), dict(segments_per_stream=2, stream_bytes=len(one)))
    if want("exchanges_x4"):
        frames = connection(exchange, (len(exchange) + 3) // 4)
        assert len(frames) == 5
        ds = flows.DNSStreams(ctx, parser, a.streams * 3)
        parts = [frames[:2], frames[2:3], frames[3:4], frames[4:]]
        calls = []
        for k, part in enumerate(parts):
            d, o, c = tiled(part, a.streams)
            r = ds.feed(d, o, c)
            last, lc = ds.asm._last, ds._last_call
            need = D.needed(r.counts)
            args = (ctx, parser, last["data"], last["offsets"], last["caplens"], last["records"], last["layouts"],
                    last["out"])
            # a tail arena of its own: the input arena of the next call stays as it is
            t_all, t_placed, t_sizing = three(ds.decoder, args, need, lc["carry"], torch.empty_like(lc["out"]["tails"]))
            tin = 0 if lc["carry"][3] is None else int(lc["carry"][3].numel())
            calls.append(dict(call=k, packets=int(last["offsets"].numel()), streams=r.counts[0], messages=r.counts[2],
                              tail_bytes_in=tin, tail_bytes_out=need[3], streams_ms=spread(t_all),
                              placed_ms=spread(t_placed), sizing_ms=spread(t_sizing)))
            print(json.dumps(calls[-1]), flush=True)
        ds.close()
        res["rows"].append(dict(case="exchanges_x4", streams=a.streams, calls=calls,
                                streams_ms_sum=sum(x["streams_ms"]["median"] for x in calls)))
    if want("zone"):
        payload = b"".join(pre(small(i)) for i in range(a.zone_messages))
        frames = connection(payload, MSS)
        stride = 1520
        rows = np.zeros((len(frames), stride), np.uint8)
        for k, f in enumerate(frames):
            rows[k, :len(f)] = np.frombuffer(f, np.uint8)
        d = torch.cat([torch.from_numpy(rows).cuda().flatten(), torch.zeros(32, dtype=torch.uint8, device="cuda")])
        caps = torch.tensor([len(f) for f in frames], dtype=torch.int32, device="cuda")
        offs = torch.arange(len(frames), dtype=torch.int64, device="cuda") * stride
        one_call("zone", d, offs, caps, dict(message_bytes=38, messages_in_the_stream=a.zone_messages))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
