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

Time is opt-in at construction. NewAssembler(pool) keeps none: FlushOlderThan
and FlushWithOptions raise, and Reassembly.Seen is whatever the caller passed
as the source packet's timestamp. NewAssembler(pool, timed=True) requires
timestamps with every batch, as an int64 array of nanoseconds
(time.Time.UnixNano(), greater than INT64_MIN) or a _lib.CAPINFO_DTYPE array;
the device then keeps every connection's lastSeen and every page's Seen
(include/gpk_tcpasm.h), Reassembly.Seen is the source packet's timestamp in
ns, and FlushOlderThan(t) / FlushWithOptions(FlushOptions(T, CloseAll)) replay
their callbacks in stream order, as FlushAll does, and return
(flushed, closed). One departure from the reference, documented in the header:
a new connection starts with no lastSeen, where the reference lets it inherit
that of the closed connection whose struct it reuses; the two agree whenever
timestamps do not run backwards.

Still out of scope: a non-zero MaxBufferedPagesTotal raises. There is no CPU
fallback.
"""
import numpy as np

from . import _lib, flows, gopacket, layers

# the decoders of examples/statsassembly (main.go:141-142)
DECODERS = (_lib.DEC_ETHERNET, _lib.DEC_DOT1Q, _lib.DEC_IPV4, _lib.DEC_IPV6, _lib.DEC_IPV6_EXT, _lib.DEC_TCP,
            _lib.DEC_PAYLOAD)
SCOPE = ("%s is out of scope: this Assembler keeps no time (NewAssembler(pool, timed=True) does, "
         "include/gpk_tcpasm.h); use FlushAll, or close old connections from Reassembly.Seen")


class Reassembly:
    """assembly.go:74-88"""
    __slots__ = ("Bytes", "Skip", "Start", "End", "Seen")

    def __init__(self, Bytes=b"", Skip=0, Start=False, End=False, Seen=None):
        self.Bytes, self.Skip, self.Start, self.End, self.Seen = Bytes, Skip, Start, End, Seen

    def __repr__(self):
        return "Reassembly(%d bytes, Skip=%d, Start=%s, End=%s)" % (len(self.Bytes), self.Skip, self.Start, self.End)


class FlushOptions:
    """assembly.go:207-210. T in int64 ns."""
    __slots__ = ("T", "CloseAll")

    def __init__(self, T=_lib.TIME_ZERO, CloseAll=False):
        self.T, self.CloseAll = T, CloseAll


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

    def __init__(self, pool, ctx=None, parser=None, max_packets=1 << 20, device=0, timed=False):
        self.connPool = pool
        self.timed = bool(timed)
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
            self._dev = flows.TCPAssembler(ctx, parser, n, device=device, keys=True, timed=self.timed)
        self._dev.max_pages = int(self.MaxBufferedPagesPerConnection)
        return self._dev

    def AssembleBatch(self, data, offsets, caplens, timestamps=None):
        """AssembleWithTimestamp (:536) for every packet of a batch, in order.
        data/offsets/caplens: numpy arrays (uint8, offsets, lengths) or device
        tensors; timestamps: one value per packet, handed back as Seen; timed: an
        int64 ns array or a _lib.CAPINFO_DTYPE array, required."""
        import torch
        dev = self._device()
        ns = None
        if self.timed:
            if timestamps is None:
                raise ValueError("a timed Assembler needs the packets' timestamps")
            ts = np.asarray(timestamps)
            if ts.dtype == _lib.CAPINFO_DTYPE:
                ts = ts["ts_sec"].astype(np.int64) * 1000000000 + ts["ts_nsec"].astype(np.int64)
            elif ts.dtype != np.int64:
                raise ValueError("timestamps: int64 nanoseconds or a CAPINFO_DTYPE array")
            timestamps = ts.tolist()
            ns = torch.from_numpy(np.ascontiguousarray(ts)).cuda()
        if not torch.is_tensor(data):
            data = torch.from_numpy(np.concatenate([np.asarray(data, np.uint8), np.zeros(16, np.uint8)])).cuda()
            offsets = torch.from_numpy(np.asarray(offsets).astype(np.int64)).cuda()
            caplens = torch.from_numpy(np.asarray(caplens).astype(np.int32)).cuda()
        bno = dev._batch
        self._seen[bno] = timestamps
        self._replay(dev.assemble(data, offsets, caplens, ns) if self.timed else dev.assemble(data, offsets, caplens))

    def FlushAll(self):
        """:279-290 -> the number of connections closed"""
        return self._replay(self._device().flush_all())

    def FlushOlderThan(self, t):
        """:272-274 -> (flushed, closed); t in int64 ns. timed=True only."""
        if not self.timed:
            raise NotImplementedError(SCOPE % "FlushOlderThan")
        return self.FlushWithOptions(FlushOptions(T=t, CloseAll=True))

    def FlushWithOptions(self, opt):
        """:238-269 -> (flushed, closed). timed=True only."""
        if not self.timed:
            raise NotImplementedError(SCOPE % "FlushWithOptions")
        res = self._device().flush_older_than(int(opt.T), close_all=bool(opt.CloseAll))
        self._replay(res)
        return res["flushed"], res["closed"]

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
