"""tcpassembly's interface (tcpassembly/assembly.go) on top of the device
reassembly (include/gpk_tcpasm.h, flows.TCPAssembler): a StreamFactory makes a
Stream per connection, the Assembler hands each stream its Reassembly objects
in order and tells it when the connection is complete.

The unit of work is a batch: AssembleBatch decodes, keys and reassembles a
whole batch on the device and then replays the result as the callbacks the
reference would have made, in its order: New at the call that created the
stream, one Reassembled(list) per Assemble call that delivered something, in
call order, ReassemblyComplete after the call that closed the connection.
FlushAll's callbacks come in stream order (the reference iterates a Go map
there, so it defines no order between connections).

Scope: no time. FlushOlderThan / FlushWithOptions and a non-zero
MaxBufferedPagesTotal raise: the device path has no counterpart (see the
header). Reassembly.Seen is the caller's timestamp of the chunk's source
packet. There is no CPU fallback.
"""
import numpy as np

from . import _lib, flows, gopacket, layers

# the decoders of examples/statsassembly (main.go:141-142)
DECODERS = (_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP,
            _lib.DEC_PAYLOAD)
SCOPE = ("%s is out of scope: the device reassembly keeps no time (include/gpk_tcpasm.h); "
         "use FlushAll, or close old connections from Reassembly.Seen")


class Reassembly:
    """assembly.go:74-88"""
    __slots__ = ("Bytes", "Skip", "Start", "End", "Seen")

    def __init__(self, Bytes=b"", Skip=0, Start=False, End=False, Seen=None):
        self.Bytes, self.Skip, self.Start, self.End, self.Seen = Bytes, Skip, Start, End, Seen

    def __repr__(self):
        return "Reassembly(%d bytes, Skip=%d, Start=%s, End=%s)" % (len(self.Bytes), self.Skip, self.Start, self.End)


class Stream:
    """assembly.go:175-184"""

    def Reassembled(self, reassembly):
        raise NotImplementedError

    def ReassemblyComplete(self):
        raise NotImplementedError


class StreamFactory:
    """assembly.go:186-193"""

    def New(self, netFlow, tcpFlow):
        raise NotImplementedError


class StreamPool:
    """NewStreamPool(factory) (:341-350). The connections live on the device,
    with the Assembler that uses the pool; one Assembler per pool."""

    def __init__(self, factory):
        self.factory = factory


def NewStreamPool(factory):
    return StreamPool(factory)


class Assembler:
    """NewAssembler(pool) (:477-486) for batches."""

    def __init__(self, pool, ctx=None, parser=None, max_packets=1 << 20, device=0):
        self.connPool = pool
        self.MaxBufferedPagesPerConnection = 0
        self.MaxBufferedPagesTotal = 0
        self._args = (ctx, parser, int(max_packets), device)
        self._dev = None
        self._streams = {}  # global stream id -> Stream
        self._seen = {}     # batch number -> timestamps

    def _device(self):
        if self.MaxBufferedPagesTotal:
            raise NotImplementedError(SCOPE % "MaxBufferedPagesTotal")
        if self._dev is None:
            from . import engine
            ctx, parser, n, device = self._args
            ctx = ctx or engine.Context(device)
            parser = parser or engine.ParserConfig(int(layers.LayerTypeEthernet), list(DECODERS))
            self._dev = flows.TCPAssembler(ctx, parser, n, device=device, keys=True)
        self._dev.max_pages = int(self.MaxBufferedPagesPerConnection)
        return self._dev

    def AssembleBatch(self, data, offsets, caplens, timestamps=None):
        """AssembleWithTimestamp (:536) for every packet of a batch, in order.
        data/offsets/caplens: numpy arrays (uint8, offsets, lengths) or device
        tensors; timestamps: one value per packet, handed back as Seen."""
        import torch
        dev = self._device()
        if not torch.is_tensor(data):
            data = torch.from_numpy(np.concatenate([np.asarray(data, np.uint8), np.zeros(16, np.uint8)])).cuda()
            offsets = torch.from_numpy(np.asarray(offsets).astype(np.int64)).cuda()
            caplens = torch.from_numpy(np.asarray(caplens).astype(np.int32)).cuda()
        bno = dev._batch
        self._seen[bno] = timestamps
        self._replay(dev.assemble(data, offsets, caplens))

    def FlushAll(self):
        """:279-290 -> the number of connections closed"""
        return self._replay(self._device().flush_all())

    def FlushOlderThan(self, t):
        raise NotImplementedError(SCOPE % "FlushOlderThan")

    def FlushWithOptions(self, opt):
        raise NotImplementedError(SCOPE % "FlushWithOptions")

    def _replay(self, res):
        # one host copy of the streams' bytes; every Reassembly.Bytes is a view of it
        blob = memoryview(res["data"][:res["counts"][2]].cpu().numpy()) if res["streams"] else memoryview(b"")
        events = []  # packet calls first, in call order; then the flush, by global stream id

        def when(call, stage, sid):
            return (1, sid, call[1], stage) if call[0] == "flush" else (0, call[1], stage, sid)

        closed = 0
        for st in res["streams"]:
            sid = st["id"]
            if st["new"]:
                net_t, src, dst, sport, dport = st["key"]
                net = gopacket.NewFlow(layers.EndpointIPv6 if net_t == 6 else layers.EndpointIPv4, src, dst)
                tr = gopacket.NewFlow(layers.EndpointTCPPort, sport, dport)
                events.append((when(st["first"], 0, sid), "new", sid, (net, tr)))
            run, last = [], None
            for ch in st["chunks"] + [None]:
                if ch is None or ch["call"] != last:
                    if run:
                        events.append((when(last, 1, sid), "data", sid, run))
                    run, last = [], None if ch is None else ch["call"]
                if ch is not None:
                    b, i = ch["src"]
                    ts = self._seen.get(b)
                    run.append(Reassembly(blob[ch["dst"]:ch["dst"] + ch["len"]], ch["skip"],
                                          bool(ch["flags"] & _lib.TCP_START), bool(ch["flags"] & _lib.TCP_END),
                                          None if ts is None else ts[i]))
            if st["closed"] is not None:
                events.append((when(st["closed"], 2, sid), "complete", sid, None))
                closed += 1
        events.sort(key=lambda e: e[0])
        for _, kind, sid, arg in events:
            if kind == "new":
                self._streams[sid] = self.connPool.factory.New(*arg)
            elif kind == "data":
                self._streams[sid].Reassembled(arg)
            else:
                self._streams.pop(sid).ReassemblyComplete()
        carry = self._dev._carry
        live = {b for b, _ in carry[6]} if carry is not None else set()
        for b in [b for b in self._seen if b not in live]:
            del self._seen[b]
        return closed

    def close(self):
        if self._dev is not None:
            self._dev.close()
            self._dev = None


def NewAssembler(pool, **kw):
    return Assembler(pool, **kw)
