#!/usr/bin/env python3
"""Read a capture, rewrite header fields, write it out: NAT, TTL and VLAN edits
of a whole capture file without a packet's bytes leaving the GPU.

A pcap or pcapng file is read in batches (pcapgo ReadBatch), each batch is
uploaded once and decoded with its layouts and layer fields
(Context.decode_device_fields). The rewrites are tensor operations on the
fields records; gopacket.SerializeBatch with FixLengths and ComputeChecksums
builds the new packets on the device (include/gpk_serialize.h: lengths and both
checksums follow the edits), and writer.WritePackets frames them. Only the
bytes of the output file come back to the host. A packet the serializer
rejects (its status is not 0) is left out and counted.

  --dnat OLD=NEW   IPv4 packets to destination OLD go to NEW
  --ttl-dec        IPv4 TTL and IPv6 HopLimit minus one (where above 0)
  --vlan-pop       drop the (innermost decoded) 802.1Q tag

The output is a nanosecond pcap file.

  python examples/pcaprewrite.py in.pcap out.pcap --dnat 10.0.0.1=192.168.1.1 --ttl-dec
"""
import argparse
import ipaddress
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ETH, D1Q, IP4, IP6 = 0, 1, 2, 3  # gpk_layout slots


def rewrite(fields, dnat=None, ttl_dec=False, vlan_pop=False):
    """The edits, in place, on the (n, 128) uint8 view of the gpk_fields records (include/gpk.h offsets)."""
    import torch
    present = fields[:, 0]
    if dnat:
        old = torch.tensor(list(ipaddress.ip_address(dnat[0]).packed), dtype=torch.uint8, device=fields.device)
        new = torch.tensor(list(ipaddress.ip_address(dnat[1]).packed), dtype=torch.uint8, device=fields.device)
        hit = ((present >> IP4) & 1).bool() & (fields[:, 52:56] == old).all(dim=1)
        fields[:, 52:56] = torch.where(hit[:, None], new[None, :], fields[:, 52:56])
    if ttl_dec:
        for slot, col in ((IP4, 27), (IP6, 46)):
            dec = ((present >> slot) & 1).bool() & (fields[:, col] > 0)
            fields[:, col] -= dec.to(torch.uint8)
    if vlan_pop:
        pop = (((present >> D1Q) & 1) & ((present >> ETH) & 1)).bool()
        fields[:, 4:6] = torch.where(pop[:, None], fields[:, 22:24], fields[:, 4:6])  # eth_type = d1q_type
        fields[:, 0] = torch.where(pop, present & (0xFF ^ (1 << D1Q)), present)


def run(inp, out, dnat=None, ttl_dec=False, vlan_pop=False, batch=1 << 16, log=print):
    """Returns (packets read, packets written, packets the serializer rejected)."""
    import numpy as np
    import torch
    from gopacket_amd import _lib, engine, gopacket, pcapgo
    read = written = rejected = 0
    ctx = engine.Context(0)
    parser = engine.ParserConfig(17, [_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6,
                                      _lib.DEC_IPV6_EXT, _lib.DEC_TCP, _lib.DEC_UDP, _lib.DEC_PAYLOAD])
    opts = gopacket.SerializeOptions(FixLengths=True, ComputeChecksums=True)
    with open(inp, "rb") as src, open(out, "wb") as dst:
        magic = src.read(4)
        src.seek(0)
        ng_in = magic == b"\x0a\x0d\x0d\x0a"
        r = pcapgo.NewNgReader(src) if ng_in else pcapgo.NewReader(src)
        w = pcapgo.NewWriterNanos(dst)
        w.WriteFileHeader(r.Snaplen() if not ng_in else (r.Interface(0).SnapLength or 262144), r.LinkType())
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
            d = torch.from_numpy(b.data).cuda()
            o = torch.from_numpy(b.offsets.astype(np.int64)).cuda()
            c = torch.from_numpy(b.caplens.astype(np.int32)).cuda()
            rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
            fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
            lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
            f = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
            ctx.decode_device_fields(parser, d, o, c, rec, err, fl, f, layouts=lay, stream=torch.cuda.current_stream())
            rewrite(f.view(n, 128), dnat, ttl_dec, vlan_pop)
            res = gopacket.SerializeBatch(opts, d, o, c, lay, f)
            # the new CaptureInfo on the device: the wire length moves with the captured length
            ci = torch.from_numpy(np.ascontiguousarray(b.ci, _lib.CAPINFO_DTYPE).view(np.int32).reshape(n, 6).copy()).cuda()
            ci[:, 3] = torch.clamp(ci[:, 3] + (res["caplens"] - c), min=0)
            ci[:, 3] = torch.maximum(ci[:, 3], res["caplens"])
            keep = torch.nonzero(res["status"] == 0).flatten().to(torch.int32)
            k = keep.numel()
            rejected += n - k
            if k:
                written += w.WritePackets(res["out"], res["offsets"][:n].contiguous(), res["caplens"],
                                          ci.view(torch.uint8).flatten(), order=keep)
        w.close()
    log("read %d packets, wrote %d, rejected %d" % (read, written, rejected))
    return read, written, rejected


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("input", help="a pcap or pcapng capture")
    ap.add_argument("output")
    ap.add_argument("--dnat", metavar="OLD=NEW", help="rewrite the IPv4 destination address OLD to NEW")
    ap.add_argument("--ttl-dec", action="store_true", help="decrement the IPv4 TTL / IPv6 HopLimit")
    ap.add_argument("--vlan-pop", action="store_true", help="drop the 802.1Q tag")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per batch")
    a = ap.parse_args()
    run(a.input, a.output, a.dnat.split("=") if a.dnat else None, a.ttl_dec, a.vlan_pop, a.batch)


if __name__ == "__main__":
    main()
