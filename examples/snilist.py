#!/usr/bin/env python3
"""List the TLS server names of a capture: per name, the packets and bytes of
the ClientHellos that carry it.

A pcap or pcapng file is read in batches (pcapgo ReadBatch). Each batch is
decoded on the device by a DecodingLayerParser that holds layers.TLS: the
six-layer decode, then the TLS pass (gpk_tls_batch) over the packets that stop
in front of LayerTypeTLS. SNIs() reads the (packet, server name) pairs from
the pass's hello entries and name arena: of the packets only those names come
back to the host. A packet's bytes are its length on the wire.

Each packet is decoded on its own, as gopacket does: a ClientHello split over
two TCP segments is not reassembled and gives no name.

  python examples/snilist.py capture.pcap
"""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(inp, parser=None, device=True, batch=1 << 16, log=print):
    """Returns {server name: [packets, bytes]}, in the order of first sight.
    parser: a DecodingLayerParser with layers.TLS (default: the Ethernet one);
    device=False runs the host entries on the calling thread."""
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
    a = ap.parse_args()
    run(a.capture, batch=a.batch)


if __name__ == "__main__":
    main()
