#!/usr/bin/env python3
"""Read a capture, keep what a classic BPF program matches, write it out: the
most common capture-tool pipeline, with the filter and the framing of the
output on the GPU.

A pcap or pcapng file is read in batches (pcapgo ReadBatch), each batch is
uploaded once, BPF.Select runs the program over it (the wire length is the
CaptureInfo's Length, as BPF.Matches takes it) and writer.WritePackets frames
the selected packets on the device, with Select's index as `order`: the batch
is never packed, and only the bytes of the output file come back to the host.

The output is pcapng (one section; the input's interfaces are carried over,
their timestamp offsets already applied by the reader) or, with --pcap, a
nanosecond pcap file.

FILE holds the program as `tcpdump -dd` prints it ("{ 0x28, 0, 0, 0x0000000c },"
per line) or as a JSON list of [code, jt, jf, k].

  python examples/pcapfilter.py in.pcapng out.pcapng --insns tcp.bpf
"""
import argparse
import dataclasses
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_insns(path):
    text = open(path).read()
    if text.lstrip().startswith("["):
        return [tuple(int(v) for v in x) for x in json.loads(text)]
    return [tuple(int(v, 0) for v in m.groups())
            for m in re.finditer(r"\{\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*\}", text)]


def run(inp, out, insns, pcap=False, batch=1 << 16, log=print):
    """Returns (packets read, packets written)."""
    import numpy as np
    import torch
    from gopacket_amd import bpf, pcapgo
    read = written = 0
    f = bpf.NewBPFInstructionFilter([bpf.BPFInstruction(*x) for x in insns])
    with open(inp, "rb") as src, open(out, "wb") as dst:
        magic = src.read(4)
        src.seek(0)
        ng_in = magic == b"\x0a\x0d\x0d\x0a"
        r = pcapgo.NewNgReader(src) if ng_in else pcapgo.NewReader(src)
        if pcap:
            w = pcapgo.NewWriterNanos(dst)
            w.WriteFileHeader(r.Snaplen() if not ng_in else (r.Interface(0).SnapLength or 262144), r.LinkType())
        elif ng_in:
            w = pcapgo.NewNgWriterInterface(dst, dataclasses.replace(r.Interface(0), TimestampOffset=0),
                                            pcapgo.DefaultNgWriterOptions)
        else:
            w = pcapgo.NewNgWriterInterface(dst, dataclasses.replace(pcapgo.DefaultNgInterface, LinkType=r.LinkType(),
                                                                     SnapLength=r.Snaplen()),
                                            pcapgo.DefaultNgWriterOptions)
        interfaces = 1
        while True:
            try:
                b = r.ReadBatch(batch)
            except pcapgo.EOFErrorGo:
                break
            except pcapgo.PcapgoError as e:
                log("error getting packet: %s" % e)
                break
            read += len(b)
            if ng_in and not pcap:  # interfaces the reader has met since the last batch
                for i in range(interfaces, r.NInterfaces()):
                    w.AddInterface(dataclasses.replace(r.Interface(i), TimestampOffset=0))
                interfaces = max(interfaces, r.NInterfaces())
            d = torch.from_numpy(b.data).cuda()
            o = torch.from_numpy(b.offsets.astype(np.int64)).cuda()
            c = torch.from_numpy(b.caplens.astype(np.int32)).cuda()
            wire = torch.from_numpy(b.ci["length"].astype(np.int64).astype(np.int32)).cuda()
            _, _, index, count = f.Select(d, o, c, wire)
            k = int(count.item())
            if k:
                written += w.WritePackets(d, o, c, b.ci, order=index[:k])
        if not pcap:
            w.Flush()
        w.close()
    f.close()
    log("read %d packets, wrote %d" % (read, written))
    return read, written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("input", help="a pcap or pcapng capture")
    ap.add_argument("output")
    ap.add_argument("--insns", required=True, help="the BPF program: tcpdump -dd output or a JSON list")
    ap.add_argument("--pcap", action="store_true", help="write a (nanosecond) pcap file instead of pcapng")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per batch")
    a = ap.parse_args()
    run(a.input, a.output, read_insns(a.insns), a.pcap, a.batch)


if __name__ == "__main__":
    main()
