#!/usr/bin/env python3
"""Measure gpk_tls_streams (include/gpk_tls_streams.h) on one GPU, beside the
gpk_tcpasm_batch call that feeds it and the per-packet gpk_tls_batch over the
same packets, all in one run.

Cases (sizes scale with --streams, default 64 Ki, and --segments, default 1 Mi):
  flights      --streams connections of a SYN and 16 segments of 1448 bytes: a
               ClientHello record of 2000 bytes (split over two segments), then
               Application Data records of 4000 bytes that straddle segments
  hellos       --segments connections of a SYN and one ClientHello record of
               1700 bytes in two segments
  flights_x4   the first case again, fed in four calls of four segments per
               connection through flows.TLSStreams: the pass with carried tails
               and seam records. Only the pass is timed there (the same call
               repeated on the state it had); the wrapper's host work is not.
  skew         one connection that holds all --segments segments: Application
               Data records of 16384 bytes, about 90 000 headers for one lane
Per case, median (min..max) over --runs timed runs after --warmup, each call
between two events, with capacities that hold everything.

  python tools/tls_streams_bench.py --out profiles/tls_streams.json
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
STRIDE = 1520  # a frame of 54 + 1448 bytes, rounded up to 16
CASES = ("flights", "hellos", "flights_x4", "skew")


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs)) if xs else None


def rec(ct, body=b"", ver=0x0303):
    return struct.pack(">BHH", ct, ver, len(body)) + body


def hello(size, name=b"bench.example"):
    """A ClientHello record of `size` bytes with a server name and a padding extension."""
    sni = struct.pack(">HHHBH", 0, len(name) + 5, len(name) + 3, 0, len(name)) + name
    fixed = 5 + 4 + 2 + 32 + 1 + 2 + 4 + 1 + 1 + 2 + len(sni) + 4
    exts = sni + struct.pack(">HH", 21, size - fixed) + bytes(size - fixed)
    body = struct.pack(">H", 0x0303) + bytes(range(32)) + b"\x00" + struct.pack(">H", 4) + b"\x13\x01\x13\x02" + \
        b"\x01\x00" + struct.pack(">H", len(exts)) + exts
    out = rec(22, b"\x01" + len(body).to_bytes(3, "big") + body)
    assert len(out) == size
    return out


def frame(payload, seq, flags=0x10):
    tcp = struct.pack(">HHIIBBHHH", 40000, 443, seq & 0xFFFFFFFF, 0, 0x50, flags, 1000, 0, 0) + payload
    ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(tcp), 1, 0, 64, 6, 0) + bytes([10, 0, 0, 1, 10, 0, 0, 2]) + tcp
    return MAC + b"\x08\x00" + ip


def connection(payload):
    """SYN, then the payload in segments of 1448 bytes."""
    return [frame(b"", 1000, 0x02)] + [frame(payload[at:at + MSS], 1001 + at) for at in range(0, len(payload), MSS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1 << 16)
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    from gopacket_amd import _lib, engine, flows

    prop = torch.cuda.get_device_properties(0)
    res = dict(device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count,
               shape="one lane per chunk for the cut, one lane per stream for the size and the emit step, a wave per tail",
               method="one process, %d timed runs after %d warm-up; each call between events; medians with min..max; "
                      "tcpasm_ms, streams_ms and per_packet_ms are of the same run and the same packets" % (a.runs, a.warmup),
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
        rows = np.zeros((len(frames), STRIDE), np.uint8)
        for k, f in enumerate(frames):
            rows[k, :len(f)] = np.frombuffer(f, np.uint8)
        d = torch.from_numpy(rows).cuda().repeat(count, 1, 1)  # [count, frames, STRIDE]
        ids = torch.arange(count, device="cuda", dtype=torch.int64)
        for b in range(3):
            d[:, :, 27 + b] = ((ids >> (16 - 8 * b)) & 255).to(torch.uint8)[:, None]
        caps = torch.tensor([len(f) for f in frames], dtype=torch.int32, device="cuda").repeat(count)
        offs = torch.arange(count * len(frames), dtype=torch.int64, device="cuda") * STRIDE
        return torch.cat([d.flatten(), torch.zeros(32, dtype=torch.uint8, device="cuda")]), offs, caps

    def per_packet_ms(d, o, c, rec_, lay):
        tld = flows.TLSDecoder(o.numel())
        out = tld.decode_all(ctx, d, o, c, rec_, lay, parser)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().numpy().view(np.uint32)
        need = flows.TLSDecoder.needed(counts)
        t = timed(lambda: tld.decode(ctx, d, o, c, rec_, lay, parser, *need, out=out))
        tld.close()
        return t, dict(candidates=int(counts[0]), ok=int(counts[1]), failed=int(counts[2]), hellos=need[1])

    def one_call(label, d, o, c, extra):
        n = o.numel()
        grouper, asm, dec = flows.Grouper(n), flows.Assembler(n), flows.TLSStreamDecoder(n)
        rec_, lay, groups, st = flows._decode_group(ctx, parser, grouper, d, o, c, flows.CONNECTION)
        ao = asm.assemble(d, o, c, rec_, lay, groups)
        t_asm = timed(lambda: asm.assemble(d, o, c, rec_, lay, groups, out_data=ao["data"], data_cap=d.numel()))
        out = dec.decode_all(ctx, parser, d, o, c, rec_, lay, ao)
        torch.cuda.synchronize()
        counts = out["counts"].cpu().tolist()
        need = flows.TLSStreamDecoder.needed(counts)
        t_tls = timed(lambda: dec.decode(ctx, parser, d, o, c, rec_, lay, ao, *need, out=out))
        t_pp, pp = per_packet_ms(d, o, c, rec_, lay)
        row = dict(case=label, packets=n, batch_bytes=int(c.sum(dtype=torch.int64).item()), streams=counts[0],
                   streams_decoded=counts[1], records=counts[2], failed_records=counts[3], hellos=counts[4],
                   sni_bytes=need[2], tail_bytes=need[3], tcpasm_ms=spread(t_asm), streams_ms=spread(t_tls),
                   per_packet_ms=spread(t_pp), per_packet=pp,
                   streams_over_tcpasm=statistics.median(t_tls) / statistics.median(t_asm), **extra)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        for h in (grouper, asm, dec):
            h.close()

    def want(label):
        return a.only in (None, label)

    app = rec(23, bytes(3995))
    flight = hello(2000) + app * 5
    flight = (flight + rec(23, bytes(16 * MSS - len(flight) - 5)))
    assert len(flight) == 16 * MSS
    if want("flights"):
        one_call("flights", *tiled(connection(flight), a.streams),
                 dict(segments_per_stream=16, hello_bytes=2000, records_per_stream=7))
    if want("hellos"):
        one_call("hellos", *tiled(connection(hello(1700)), a.segments), dict(segments_per_stream=2, hello_bytes=1700))
    if want("flights_x4"):
        frames = connection(flight)
        ts = flows.TLSStreams(ctx, parser, a.streams * 6)
        parts = [frames[:5], frames[5:9], frames[9:13], frames[13:]]
        calls = []
        for k, part in enumerate(parts):
            d, o, c = tiled(part, a.streams)
            r = ts.feed(d, o, c)
            last, lc = ts.asm._last, ts._last_call
            need = flows.TLSStreamDecoder.needed(r.counts)
            out = lc["out"]
            spare = dict(out, tails=torch.empty_like(out["tails"]))  # the input arena of the next call stays as it is
            t = timed(lambda: ts.decoder.decode(ctx, parser, last["data"], last["offsets"], last["caplens"],
                                                last["records"], last["layouts"], last["out"], *need, carry=lc["carry"],
                                                out=spare))
            tin = 0 if lc["carry"][3] is None else int(lc["carry"][3].numel())
            calls.append(dict(call=k, packets=int(last["offsets"].numel()), streams=r.counts[0], records=r.counts[2],
                              hellos=r.counts[4], tail_bytes_in=tin, tail_bytes_out=need[3], streams_ms=spread(t)))
            print(json.dumps(calls[-1]), flush=True)
        ts.close()
        res["rows"].append(dict(case="flights_x4", streams=a.streams, calls=calls,
                                streams_ms_sum=sum(x["streams_ms"]["median"] for x in calls)))
    if want("skew"):
        n = a.segments
        body = 16384
        payload = torch.zeros(n * MSS, dtype=torch.uint8, device="cuda")
        at = torch.arange(0, n * MSS - 5, body + 5, device="cuda")
        nrec = int(at.numel())
        lastlen = n * MSS - int(at[-1].item()) - 5
        payload[at], payload[at + 1], payload[at + 2] = 23, 3, 3
        lens = torch.full((nrec,), body, device="cuda")
        lens[-1] = min(lastlen, body)
        payload[at + 3], payload[at + 4] = (lens >> 8).to(torch.uint8), (lens & 255).to(torch.uint8)
        head = np.frombuffer(frame(bytes(MSS), 0)[:54], np.uint8)
        rows = torch.zeros((n + 1, STRIDE), dtype=torch.uint8, device="cuda")
        rows[:, :54] = torch.from_numpy(head.copy()).cuda()
        rows[1:, 54:54 + MSS] = payload.view(n, MSS)
        seq = 1001 + torch.arange(n, device="cuda", dtype=torch.int64) * MSS
        for b in range(4):
            rows[1:, 38 + b] = ((seq >> (24 - 8 * b)) & 255).to(torch.uint8)
        syn = np.frombuffer(frame(b"", 1000, 0x02), np.uint8)
        rows[0, :54] = torch.from_numpy(syn.copy()).cuda()
        caps = torch.full((n + 1,), 54 + MSS, dtype=torch.int32, device="cuda")
        caps[0] = 54
        offs = torch.arange(n + 1, dtype=torch.int64, device="cuda") * STRIDE
        d = torch.cat([rows.flatten(), torch.zeros(32, dtype=torch.uint8, device="cuda")])
        del rows, payload
        one_call("skew", d, offs, caps, dict(record_bytes=body + 5, records_in_the_stream=nrec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
