#!/usr/bin/env python3
"""List the DNS messages of a capture that travel over TCP: per TCP stream its
queries and the answer counts of its responses, with the UDP messages of the
same capture beside them.

A pcap or pcapng file is read in batches (pcapgo ReadBatch). Over TCP a DNS
message follows two length bytes and may span segments, so a packet at a time
cannot decode it: the per-packet pass reads the length bytes as the ID, as
gopacket does. Here the TCP streams are reassembled on the device
(flows.DNSStreams: gpk_tcpasm_batch, then gpk_dns_streams over every stream's
bytes), every message is framed by its length and decoded whole, and an
unfinished message waits for the next batch. The UDP messages come from the
per-packet pass (a DecodingLayerParser that holds layers.DNS). Of the packets
only the message tables and the names come back to the host.

  python examples/dnstcp.py capture.pcap
"""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _row(t, names):
    """(is a response, ID, answers, question names) of a decoded message."""
    return bool(int(t["flags2"]) & 0x80), int(t["id"]), int(t["ancount"]), names


def run(inp, ctx=None, parser=None, packet_parser=None, batch=1 << 16, max_message=0, log=print):
    """Returns dict(streams={global stream id: [(response?, ID, answers,
    [question names])]}, udp=[(packet number, response?, ID, answers,
    [question names])], failed=messages over TCP that did not decode), the
    streams in the order of first sight. parser: an engine.ParserConfig for
    the reassembly (default: the Ethernet one); packet_parser: a
    DecodingLayerParser with layers.DNS for the UDP messages."""
    import torch
    from gopacket_amd import engine, flows, gopacket as G, layers as L, pcapgo
    ctx = ctx or engine.Context(0)
    if parser is None:
        parser = engine.ParserConfig(17, [engine.DECODER_KINDS[k] for k in (  # LayerTypeEthernet
            "Ethernet", "Dot1Q", "IPv4", "IPv6", "IPv6ExtensionSkipper", "TCP", "UDP", "Payload")])
    if packet_parser is None:
        packet_parser = G.DecodingLayerParser(L.LayerTypeEthernet, L.Ethernet(), L.Dot1Q(), L.IPv4(), L.IPv6(),
                                              L.IPv6ExtensionSkipper(), L.TCP(), L.UDP(), G.Payload(), L.DNS())
    ds = flows.DNSStreams(ctx, parser, batch, max_message=max_message)
    streams, udp = collections.OrderedDict(), []
    failed = [0]

    def take(res):
        per = {}
        for g, name, _ in res.questions():
            per.setdefault(g, []).append(name)
        for s in res.streams:
            names = iter(per.get(s["id"], ()))
            for m in s["msgs"]:
                t = m["msg"]
                if int(m["status"]) or int(t["err"]):
                    failed[0] += int(t["err"]) != 0
                    continue
                streams.setdefault(s["id"], []).append(_row(t, [next(names) for _ in range(int(t["qdcount"]))]))
    seen = 0
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
            take(ds.feed(data, torch.as_tensor(b.offsets.astype("int64")).cuda(),
                         torch.as_tensor(b.caplens.astype("int32")).cuda()))
            res = packet_parser.DecodeBatch(G.PacketBatch(b.data, b.offsets, b.caplens))
            for i in range(len(b.caplens)):
                d = res.DNS(i)
                if d is None or int(d[0]["err"]) or L.LayerTypeUDP not in res.Decoded(i):
                    continue
                t, rrs, arena = d
                names = [bytes(arena[int(q["name_off"]):int(q["name_off"]) + int(q["name_len"])])
                         for q in rrs[:int(t["qdcount"])]]
                udp.append((seen + i,) + _row(t, names))
            seen += len(b.caplens)
    take(ds.flush_all())
    ds.close()

    def text(row):
        resp, ident, answers, names = row
        what = "response %5d answers" % answers if resp else "query"
        return "%04x %-22s %s" % (ident, what, ", ".join(n.decode("ascii", "backslashreplace") for n in names))
    for g, rows in streams.items():
        log("tcp stream %d: %d queries, %d responses" % (g, sum(not r[0] for r in rows), sum(r[0] for r in rows)))
        for row in rows:
            log("    " + text(row))
    log("udp: %d messages" % len(udp))
    for row in udp:
        log("    packet %-8d %s" % (row[0], text(row[1:])))
    if failed[0]:
        log("tcp: %d messages did not decode" % failed[0])
    return dict(streams=streams, udp=udp, failed=failed[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("capture", help="a pcap or pcapng capture")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per batch")
    ap.add_argument("--max-message", type=int, default=0,
                    help="skip messages longer than this many bytes (0: no limit); bounds the work of crafted names")
    a = ap.parse_args()
    run(a.capture, batch=a.batch, max_message=a.max_message)


if __name__ == "__main__":
    main()
