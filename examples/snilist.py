#!/usr/bin/env python3
"""List the TLS server names of a capture: per name, the packets and bytes of
the ClientHellos that carry it.

A pcap or pcapng file is read in batches (pcapgo ReadBatch). Each batch is
decoded on the device by a DecodingLayerParser that holds layers.TLS: the
six-layer decode, then the TLS pass (gpk_tls_batch) over the packets that stop
in front of LayerTypeTLS. SNIs() reads the (packet, server name) pairs from
the pass's hello entries and name arena: of the packets only those names come
back to the host. A packet's bytes are its length on the wire.

By default each packet is decoded on its own, as gopacket does: a ClientHello
split over two TCP segments fails there and gives no name. With --streams the
TCP streams are reassembled on the device first (flows.TLSStreams:
gpk_tcpasm_batch, then gpk_tls_streams over every stream's bytes), so a
ClientHello larger than one segment is decoded from its whole record; names
are then listed per stream: the count is of ClientHellos and no bytes are
counted, since a record belongs to no single packet.

  python examples/snilist.py capture.pcap
  python examples/snilist.py --streams capture.pcap
"""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_streams(inp, ctx=None, parser=None, batch=1 << 16, log=print):
    """Returns {server name: [ClientHellos, streams]}, in the order of first
    sight, from the reassembled streams of the capture (device only). parser:
    an engine.ParserConfig (default: the Ethernet one)."""
    import torch
    from gopacket_amd import engine, flows, pcapgo
    ctx = ctx or engine.Context(0)
    if parser is None:
        parser = engine.ParserConfig(17, [engine.DECODER_KINDS[k] for k in (  # LayerTypeEthernet
            "Ethernet", "Dot1Q", "IPv4", "IPv6", "IPv6ExtensionSkipper", "TCP", "UDP", "Payload")])
    ts = flows.TLSStreams(ctx, parser, batch)
    seen, ids = collections.OrderedDict(), {}

    def take(res):
        for g, name in res.snis():
            row = seen.setdefault(name, [0, 0])
            row[0] += 1
            if g not in ids.setdefault(name, set()):
                ids[name].add(g)
                row[1] += 1
    with open(inp, "rb") as src:
        magic = src.read(4)
        src.seek(0)
        r = pcapgo.NewNgReader(src) if magic == b"\x0a\x0d\x0d\x0a" else pcapgo.NewReader(src)
        while True:
            try:
                b = r.ReadBatch(batch)
            except pcapgo.EOFErrorGo:
                break
            except pcapgo.PcapgoError as e:
                log("error getting packet: %s" % e)
                break
            # 16 spare bytes: the byte mover's aligned loads may reach past the last payload
            data = torch.cat([torch.as_tensor(b.data, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)]).cuda()
            take(ts.feed(data, torch.as_tensor(b.offsets.astype("int64")).cuda(),
                         torch.as_tensor(b.caplens.astype("int32")).cuda()))
    take(ts.flush_all())
    ts.close()
    for name, (hellos, streams) in seen.items():
        log("%-48s %8d hellos  %10d streams" % (name.decode("ascii", "backslashreplace"), hellos, streams))
    return seen


def run(inp, parser=None, device=True, batch=1 << 16, log=print, streams=False, ctx=None):
    """Returns {server name: [packets, bytes]}, in the order of first sight.
    parser: a DecodingLayerParser with layers.TLS (default: the Ethernet one);
    device=False runs the host entries on the calling thread. streams=True:
    run_streams (the reassembly runs on the device only)."""
    if streams:
        if not device:
            raise NotImplementedError("streams=True reassembles on the device: there is no host reassembler")
        return run_streams(inp, ctx=ctx, parser=parser, batch=batch, log=log)
    from gopacket_amd import gopacket as G, layers as L, pcapgo
    if parser is None:
        parser = G.DecodingLayerParser(L.LayerTypeEthernet, L.Ethernet(), L.Dot1Q(), L.IPv4(), L.IPv6(),
                                       L.IPv6ExtensionSkipper(), L.TCP(), L.UDP(), G.Payload(), L.TLS())
    seen = collections.OrderedDict()
    with open(inp, "rb") as src:
        magic = src.read(4)
        src.seek(0)
        r = pcapgo.NewNgReader(src) if magic == b"\x0a\x0d\x0d\x0a" else pcapgo.NewReader(src)
        while True:
            try:
                b = r.ReadBatch(batch)
            except pcapgo.EOFErrorGo:
                break
            except pcapgo.PcapgoError as e:
                log("error getting packet: %s" % e)
                break
            pb = G.PacketBatch(b.data, b.offsets, b.caplens)
            res = parser.DecodeBatch(pb) if device else G.TunnelBatchResult(parser, pb, device=False)
            for i, name in res.SNIs():
                row = seen.setdefault(name, [0, 0])
                row[0] += 1
                row[1] += int(b.ci["length"][i])
    for name, (packets, nbytes) in seen.items():
        log("%-48s %8d packets %10d bytes" % (name.decode("ascii", "backslashreplace"), packets, nbytes))
    return seen


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("capture", help="a pcap or pcapng capture")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per batch")
    ap.add_argument("--streams", action="store_true", help="reassemble the TCP streams first and list names per stream")
    a = ap.parse_args()
    run(a.capture, batch=a.batch, streams=a.streams)


if __name__ == "__main__":
    main()
