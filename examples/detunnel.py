#!/usr/bin/env python3
"""Strip VXLAN / Geneve / GRE encapsulation from a capture: write the inner
Ethernet frames of its tunnelled packets, with their capture info.

A pcap or pcapng file is read in batches (pcapgo ReadBatch); each batch is
uploaded once and decoded on the device, Detunneler.peel decodes the tunnel
headers and hands back the inner slices (in_offsets / in_caplens into the same
buffer), and writer.WritePackets frames those slices: the encapsulation is
stripped without moving a packet byte, and only the bytes of the output file
come back to the host. A frame keeps its packet's timestamp and interface; its
Length is the packet's Length less the bytes stripped.

One level is peeled. Packets whose tunnel does not carry an Ethernet frame
(GRE over IPv4, say), or whose tunnel header does not decode, are dropped;
--keep-plain passes the untunnelled packets through, in capture order.

  python examples/detunnel.py in.pcapng out.pcapng [--keep-plain]
"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(inp, out, keep_plain=False, pcap=False, batch=1 << 16, log=print):
    """Returns (packets read, frames written)."""
    import numpy as np
    import torch
    from gopacket_amd import _lib, engine, flows, pcapgo
    read = written = 0
    ctx = engine.Context(0)
    parser = engine.ParserConfig(17, [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6,
                                      _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP, _lib.DEC_PAYLOAD],
                                 outputs=0)
    det = flows.Detunneler(batch)
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
            n = len(b)
            read += n
            if ng_in and not pcap:
                for i in range(interfaces, r.NInterfaces()):
                    w.AddInterface(dataclasses.replace(r.Interface(i), TimestampOffset=0))
                interfaces = max(interfaces, r.NInterfaces())
            d = torch.from_numpy(np.concatenate([b.data, np.zeros(-len(b.data) % 16 + 16, np.uint8)])).cuda()
            o = torch.from_numpy(b.offsets.astype(np.int64)).cuda()
            c = torch.from_numpy(b.caplens.astype(np.int32)).cuda()
            rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
            ctx.decode_device(parser, d, o, c, rec, None, None, lay)
            t = det.peel(ctx, d, o, c, rec, lay, parser, gre_checksum=False)
            cs = t["class_start"][:2].cpu().tolist()
            v = t["verdict"]
            inner = (v >= cs[0]) & (v < cs[1])  # GPK_TUN_CLASS_ETHERNET: the inner slice is an Ethernet frame
            keep = inner | (v < 0) if keep_plain else inner
            at = v.clamp(min=0).long()
            new_o = torch.where(inner, t["in_offsets"][at], o)
            new_c = torch.where(inner, t["in_caplens"][at], c)
            order = torch.nonzero(keep).flatten().int()
            if order.numel():
                ci = b.ci.copy()
                stripped = (c - new_c).cpu().numpy().astype(np.int64)
                ci["length"] = np.maximum(ci["length"].astype(np.int64) - stripped, new_c.cpu().numpy()).astype(np.uint32)
                written += w.WritePackets(d, new_o, new_c, ci, order=order)
        if not pcap:
            w.Flush()
        w.close()
    det.close()
    log("read %d packets, wrote %d frames" % (read, written))
    return read, written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("input", help="a pcap or pcapng capture")
    ap.add_argument("output")
    ap.add_argument("--keep-plain", action="store_true", help="pass untunnelled packets through")
    ap.add_argument("--pcap", action="store_true", help="write a (nanosecond) pcap file instead of pcapng")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per batch")
    a = ap.parse_args()
    run(a.input, a.output, a.keep_plain, a.pcap, a.batch)


if __name__ == "__main__":
    main()
