#!/usr/bin/env python3
"""The reference's examples/statsassembly loop (main.go:128-209) over a capture
file, with the decode on the GPU.

The reference reads one packet at a time from a pcap handle, decodes it with
a DecodingLayerParser of Ethernet, Dot1Q, IPv4, IPv6, IPv6ExtensionSkipper,
TCP and Payload, takes the network flow of the last IPv4/IPv6 layer before
TCP, and hands the packet to tcpassembly. tcpassembly drops "useless" packets
(no SYN, FIN or RST and no payload, tcpassembly/assembly.go:537-543) and keys
the rest by key{netFlow, tcp.TransportFlow()} (:546).

Here a pcap or pcapng file is read in batches (pcapgo ReadBatch: the packets
the next ReadPacketData calls would return), each batch is decoded in one
launch (DecodingLayerParser.DecodeBatch), and the per-packet loop is the
reference's, over the layer structs as DecodeLayers leaves them (Hydrate).
The streams' statistics stand in for statsStream's (main.go:52-99): packets,
payload bytes, first and last capture time, and whether a SYN or a FIN/RST
was seen. This default mode does not reassemble, so it has no out-of-order or
skip counts; --device-assembly (below) does.

--device-groups also forms the connection keys on the device
(gpk_group_batch, GPK_GROUP_CONNECTION) and checks that they split the
assembled packets exactly as the loop's keys do.

--device-assembly runs tcpassembly itself on the device instead
(gopacket_amd.tcpassembly, include/gpk_tcpasm.h): the statsStream objects of
main.go:52-99 are fed the reassembled chunks batch by batch, FlushAll() follows
the last batch (main.go:210), and the statistics gain the reference's
out-of-order and skipped counts. Reassembly.Seen is the capture time of the
chunk's source packet.

--flush-older-than SECONDS (with --device-assembly) is the reference's periodic
flush (main.go:156-161: every so often, FlushOlderThan(now - 2 minutes)) in
capture time, because a wall-clock trigger over a file is not reproducible:
before each batch, FlushOlderThan(first timestamp of the batch - SECONDS) runs
on the device (a timed Assembler, include/gpk_tcpasm.h), so connections that
went quiet are flushed and closed while the file is read, not only at the end.

  python examples/statsassembly.py tests/golden/test_ethernet.pcap -v
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StatsStream:
    """main.go:52-57, without the reassembly's ordering state."""

    def __init__(self, net, transport, seen):
        self.net, self.transport = net, transport
        self.bytes = self.packets = 0
        self.start = self.end = seen
        self.sawStart = self.sawEnd = False

    def assemble(self, tcp, seen):
        self.packets += 1
        self.bytes += len(tcp.LayerPayload())
        self.end = max(self.end, seen)
        self.sawStart = self.sawStart or tcp.SYN
        self.sawEnd = self.sawEnd or tcp.FIN or tcp.RST


def open_reader(f):
    from gopacket_amd import pcapgo
    magic = f.read(4)
    f.seek(0)
    return pcapgo.NewNgReader(f) if magic == b"\x0a\x0d\x0d\x0a" else pcapgo.NewReader(f)


def run(path, count=-1, batch=1 << 16, verbose=False, device_groups=False, log=print):
    """Returns (streams in order of first appearance, packets read, bytes of
    the packets decoded without error)."""
    from gopacket_amd import gopacket, layers, pcapgo
    eth, dot1q, ip4, ip6 = layers.Ethernet(), layers.Dot1Q(), layers.IPv4(), layers.IPv6()
    ip6extensions, tcp, payload = layers.IPv6ExtensionSkipper(), layers.TCP(), gopacket.Payload()
    parser = gopacket.NewDecodingLayerParser(layers.LayerTypeEthernet, eth, dot1q, ip4, ip6, ip6extensions, tcp,
                                             payload)
    decoded = []
    streams = {}  # key{netFlow, TransportFlow} -> StatsStream; dict order = the order streams were created
    read = byte_count = 0
    start = time.time()
    with open(path, "rb") as f:
        r = open_reader(f)
        while count != 0:
            try:
                b = r.ReadBatch(batch if count < 0 else min(batch, count))
            except pcapgo.EOFErrorGo:
                break
            except pcapgo.PcapgoError as e:  # the reference logs it and reads on; a file reader is done here
                log("error getting packet: %s" % e)
                break
            first = read
            read += len(b)
            if count > 0:
                count -= len(b)
            pb = gopacket.PacketBatch(b.data, b.offsets, b.caplens)
            res = parser.DecodeBatch(pb, layouts=True)
            assembled = []
            for i in range(len(pb)):
                err = res.Hydrate(i, decoded)
                if err is not None:
                    log("error decoding packet: %s" % err.Error())
                    continue
                if verbose:
                    log("decoded the following layers: [%s]" % " ".join(t.String() for t in decoded))
                byte_count += int(pb.caplens[i])
                seen = int(b.ci[i]["ts_sec"]) + int(b.ci[i]["ts_nsec"]) * 1e-9
                found_net, net_flow = False, None
                for typ in decoded:
                    if typ == layers.LayerTypeIPv4:
                        net_flow, found_net = ip4.NetworkFlow(), True
                    elif typ == layers.LayerTypeIPv6:
                        net_flow, found_net = ip6.NetworkFlow(), True
                    elif typ == layers.LayerTypeTCP:
                        if not found_net:
                            log("could not find IPv4 or IPv6 layer, inoring")
                        elif tcp.SYN or tcp.FIN or tcp.RST or len(tcp.LayerPayload()):  # assembly.go:537-543
                            key = (net_flow, tcp.TransportFlow())
                            s = streams.get(key)
                            if s is None:
                                log("new stream %s:%s started" % (key[0], key[1]))
                                s = streams[key] = StatsStream(key[0], key[1], seen)
                            s.assemble(tcp, seen)
                            assembled.append((i, key))
                        break
                else:
                    log("could not find TCP layer")
            if device_groups:
                check_device_groups(parser, pb, assembled)
    for s in streams.values():
        secs = s.end - s.start
        log("Reassembly of stream %s:%s complete - start:%.6f end:%.6f bytes:%d packets:%d bps:%s pps:%s "
            "sawStart:%s sawEnd:%s" % (s.net, s.transport, s.start, s.end, s.bytes, s.packets,
                                       "%.1f" % (s.bytes / secs) if secs > 0 else "+Inf",
                                       "%.1f" % (s.packets / secs) if secs > 0 else "+Inf",
                                       str(s.sawStart).lower(), str(s.sawEnd).lower()))
    log("processed %d bytes in %.3fs" % (byte_count, time.time() - start))
    return list(streams.values()), read, byte_count


class DeviceStatsStream:
    """statsStream (main.go:52-99) as a gopacket_amd.tcpassembly Stream. start
    is the capture time of the first chunk (the reference takes time.Now() in
    New, which a capture file cannot give)."""

    def __init__(self, net, transport, log, unit=1.0):
        self.net, self.transport, self.log = net, transport, log
        self.unit = unit  # seconds per unit of Reassembly.Seen (a timed Assembler hands back int64 ns)
        self.bytes = self.packets = self.outOfOrder = self.skipped = 0
        self.start = self.end = None
        self.sawStart = self.sawEnd = self.complete = False

    def Reassembled(self, reassemblies):
        for r in reassemblies:
            seen = r.Seen * self.unit
            if self.start is None:
                self.start = self.end = seen
            if seen < self.end:
                self.outOfOrder += 1
            else:
                self.end = seen
            self.bytes += len(r.Bytes)
            self.packets += 1
            if r.Skip > 0:
                self.skipped += r.Skip
            self.sawStart = self.sawStart or r.Start
            self.sawEnd = self.sawEnd or r.End

    def ReassemblyComplete(self):
        self.complete = True
        secs = (self.end - self.start) if self.start is not None else 0
        self.log("Reassembly of stream %s:%s complete - start:%s end:%s bytes:%d packets:%d ooo:%d bps:%s pps:%s "
                 "skipped:%d" % (self.net, self.transport, "%.6f" % self.start if self.start is not None else "-",
                                 "%.6f" % self.end if self.end is not None else "-", self.bytes, self.packets,
                                 self.outOfOrder, "%.1f" % (self.bytes / secs) if secs > 0 else "+Inf",
                                 "%.1f" % (self.packets / secs) if secs > 0 else "+Inf", self.skipped))


def run_device_assembly(path, count=-1, batch=1 << 16, max_pages=0, log=print, flush_older_than=None):
    """main.go:119-211 with tcpassembly on the device. Returns (streams in the
    order of their New calls, packets read, bytes of the packets decoded
    without error). flush_older_than: seconds; before each batch
    FlushOlderThan(the batch's first timestamp - flush_older_than) runs, the
    capture-time form of main.go:156-161."""
    import numpy as np
    from gopacket_amd import _lib, gopacket, layers, pcapgo, tcpassembly
    parser = gopacket.NewDecodingLayerParser(layers.LayerTypeEthernet, layers.Ethernet(), layers.Dot1Q(),
                                             layers.IPv4(), layers.IPv6(), layers.IPv6ExtensionSkipper(), layers.TCP(),
                                             gopacket.Payload())
    made = []

    class Factory(tcpassembly.StreamFactory):
        def New(self, net, transport):
            log("new stream %s:%s started" % (net, transport))
            made.append(DeviceStatsStream(net, transport, log, 1e-9 if timed else 1.0))
            return made[-1]

    timed = flush_older_than is not None
    assembler = tcpassembly.NewAssembler(tcpassembly.NewStreamPool(Factory()), ctx=parser.ctx(),
                                         parser=parser._config(), max_packets=2 * batch + 1024, timed=timed)
    assembler.MaxBufferedPagesPerConnection = max_pages
    read = byte_count = 0
    start = time.time()
    with open(path, "rb") as f:
        r = open_reader(f)
        while count != 0:
            try:
                b = r.ReadBatch(batch if count < 0 else min(batch, count))
            except pcapgo.EOFErrorGo:
                break
            except pcapgo.PcapgoError as e:
                log("error getting packet: %s" % e)
                break
            read += len(b)
            if count > 0:
                count -= len(b)
            pb = gopacket.PacketBatch(b.data, b.offsets, b.caplens)
            res = parser.DecodeBatch(pb)
            # the loop `continue`s on a decode error (main.go:179-182): those packets are not assembled
            ok = np.flatnonzero((res.records["status"] & _lib.ST_ERR_MASK) == 0)
            for i in np.flatnonzero((res.records["status"] & _lib.ST_ERR_MASK) != 0):
                log("error decoding packet: %s" % res.Err(int(i)).Error())
            byte_count += int(pb.caplens[ok].sum())
            if timed:
                seen = b.ci["ts_sec"][ok].astype(np.int64) * 1000000000 + b.ci["ts_nsec"][ok].astype(np.int64)
                if len(seen):
                    flushed, closed = assembler.FlushOlderThan(int(seen[0]) - int(flush_older_than * 1e9))
                    log("forced flush: %d flushed, %d closed" % (flushed, closed))  # main.go:159-160
            else:
                seen = b.ci["ts_sec"][ok].astype(np.float64) + b.ci["ts_nsec"][ok] * 1e-9
            assembler.AssembleBatch(pb.data, pb.offsets[ok], pb.caplens[ok], seen)
    assembler.FlushAll()
    assembler.close()
    log("processed %d bytes in %.3fs" % (byte_count, time.time() - start))
    return made, read, byte_count


def check_device_groups(parser, pb, assembled):
    """The same batch decoded and grouped on the device (gpk_group_batch,
    CONNECTION): every key of the loop must be exactly one device group and
    no two keys one group. The device also keys packets whose decode failed
    after TCP; the loop skips those (DecodeLayers returned an error), so only
    the loop's packets are compared."""
    import numpy as np
    import torch
    from gopacket_amd import flows
    n = len(pb)
    d = torch.from_numpy(np.concatenate([pb.data, np.zeros(16, np.uint8)])).cuda()
    o = torch.from_numpy(pb.offsets.astype(np.int64)).cuda()
    c = torch.from_numpy(pb.caplens.astype(np.int32)).cuda()
    rec = torch.empty(16 * n, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.empty(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    parser.ctx().decode_device(parser._config(), d, o, c, rec, err, fl, lay)
    g = flows.Grouper(max(n, 1))
    group_of = g.group(d, o, c, rec, layouts=lay, flows=fl, kind=flows.CONNECTION)["group_of"].cpu().numpy()
    g.close()
    key_of_group = {}
    group_of_key = {}
    for i, key in assembled:
        gid = int(group_of[i])
        if gid < 0 or key_of_group.setdefault(gid, key) != key or group_of_key.setdefault(key, gid) != gid:
            raise AssertionError("packet %d: device group %d, loop key %s:%s" % (i, gid, key[0], key[1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("file", help="a pcap or pcapng capture")
    ap.add_argument("-c", type=int, default=-1, help="quit after this many packets (negative: all)")
    ap.add_argument("-v", action="store_true", help="log every packet's decoded layers")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per DecodeBatch launch")
    ap.add_argument("--device-groups", action="store_true",
                    help="also group on the device (gpk_group_batch) and check it against the loop")
    ap.add_argument("--device-assembly", action="store_true",
                    help="reassemble the TCP streams on the device (gopacket_amd.tcpassembly)")
    ap.add_argument("--max-pages", type=int, default=0,
                    help="MaxBufferedPagesPerConnection for --device-assembly (0: no limit)")
    ap.add_argument("--flush-older-than", type=float, default=None, metavar="SECONDS",
                    help="with --device-assembly: before each batch, FlushOlderThan(its first timestamp - SECONDS)")
    a = ap.parse_args()
    if a.flush_older_than is not None and not a.device_assembly:
        ap.error("--flush-older-than needs --device-assembly")
    if a.device_assembly:
        run_device_assembly(a.file, a.c, a.batch, a.max_pages, flush_older_than=a.flush_older_than)
        return
    run(a.file, a.c, a.batch, a.v, a.device_groups)


if __name__ == "__main__":
    main()
