"""Flow-keyed grouping of a decoded batch on the device (include/gpk_flows.h,
SURVEY.md §8(f)3): the keying the reference's flow consumers do per packet
with a Go map, for a whole batch in HBM.

  Grouper(max_packets).group(...)          gpk_group_batch
  kind CONNECTION                          tcpassembly key{netFlow, TransportFlow()}
                                           (tcpassembly/assembly.go:292,525-545)
  kind DEFRAG                              ip4defrag ipv4{NetworkFlow(), Id}
                                           (ip4defrag/defrag.go:85-105,328-341)
  kind NET_BUCKET                          int(NetworkFlow().FastHash()) & (buckets-1)
                                           (doc.go:219-225)

Groups come in order of first appearance; packets inside a group in batch
order. group_of[i] < 0 says why packet i has no key (GROUP_* codes).

  Defragmenter(max_packets).defrag(...)    gpk_defrag_batch (include/gpk_defrag.h):
                                           ip4defrag's reassembly of a DEFRAG-grouped
                                           batch (defrag.go:113-132,214-326)
  IPv4Defragmenter(ctx, parser, n)         the same over a stream of batches
"""
import ctypes

from . import _lib

CONNECTION, DEFRAG, NET_BUCKET = _lib.GROUP_CONNECTION, _lib.GROUP_DEFRAG, _lib.GROUP_NET_BUCKET
NONE, USELESS, FRAG_TOO_SMALL, FRAG_OFFSET, FRAG_OVERRUN, UNKNOWN = (
    _lib.GROUP_NONE, _lib.GROUP_USELESS, _lib.GROUP_FRAG_TOO_SMALL, _lib.GROUP_FRAG_OFFSET,
    _lib.GROUP_FRAG_OVERRUN, _lib.GROUP_UNKNOWN)


class Grouper:
    def __init__(self, max_packets, device=0):
        self.h = ctypes.c_void_p()
        _lib.check(_lib.lib().gpk_grouper_create(ctypes.byref(self.h), device, int(max_packets)))
        self.max_packets = int(max_packets)

    def group(self, data, offsets, caplens, records, layouts=None, flows=None, kind=CONNECTION, buckets=8,
              out=None, stream=None):
        """Device tensors in (torch, as gpk_decode_batch takes them); returns
        dict(group_of, perm, start, first, counts) of device tensors (or fills `out`)."""
        import torch
        n = offsets.numel()
        dev = offsets.device
        if out is None:
            out = dict(group_of=torch.empty(n, dtype=torch.int32, device=dev),
                       perm=torch.empty(n, dtype=torch.int32, device=dev),
                       start=torch.empty(n + 1, dtype=torch.int32, device=dev),
                       first=torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                       counts=torch.zeros(2, dtype=torch.int32, device=dev))
        b = _lib.Batch(data.data_ptr(), offsets.data_ptr(), caplens.data_ptr(), n, data.numel())
        r = _lib.Results(records.data_ptr(), None, flows.data_ptr() if flows is not None else None,
                         layouts.data_ptr() if layouts is not None else None)
        g = _lib.Groups(out["group_of"].data_ptr(), out["perm"].data_ptr(), out["start"].data_ptr(),
                        out["first"].data_ptr(), out["counts"].data_ptr())
        sp = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        _lib.check(_lib.lib().gpk_group_batch(self.h, ctypes.byref(b), ctypes.byref(r), int(kind), int(buckets),
                                              ctypes.byref(g), sp))
        return out

    def decode_group(self, ctx, parser, data, offsets, caplens, records, err_args=None, flows=None, kind=CONNECTION,
                     out=None, stream=None):
        """gpk_decode_group_batch: decode (records/err_args/flows as
        Context.decode_device, no layouts) and group by `kind` (CONNECTION or
        DEFRAG) with the key derived inside the decode kernel."""
        import torch
        n = offsets.numel()
        dev = offsets.device
        if out is None:
            out = dict(group_of=torch.empty(n, dtype=torch.int32, device=dev),
                       perm=torch.empty(n, dtype=torch.int32, device=dev),
                       start=torch.empty(n + 1, dtype=torch.int32, device=dev),
                       first=torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                       counts=torch.zeros(2, dtype=torch.int32, device=dev))
        b = _lib.Batch(data.data_ptr(), offsets.data_ptr(), caplens.data_ptr(), n, data.numel())
        r = _lib.Results(records.data_ptr(), err_args.data_ptr() if err_args is not None else None,
                         flows.data_ptr() if flows is not None else None, None)
        g = _lib.Groups(out["group_of"].data_ptr(), out["perm"].data_ptr(), out["start"].data_ptr(),
                        out["first"].data_ptr(), out["counts"].data_ptr())
        sp = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        _lib.check(_lib.lib().gpk_decode_group_batch(ctx.h, parser.h, ctypes.byref(b), ctypes.byref(r), self.h,
                                                     int(kind), ctypes.byref(g), sp))
        return out

    @staticmethod
    def to_lists(out):
        """Host view: (groups: list of packet-index lists in group order, group_of list)."""
        counts = out["counts"].cpu().tolist()
        G, K = counts[0], counts[1]
        perm = out["perm"][:K].cpu().tolist()
        start = out["start"][:G + 1].cpu().tolist()
        return [perm[start[g]:start[g + 1]] for g in range(G)], out["group_of"].cpu().tolist()

    def close(self):
        if self.h:
            _lib.lib().gpk_grouper_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_batch(data, offsets, caplens, order, total_bytes=None, stream=None):
    """gpk_pack_batch: the packets `order` (device int32 tensor) of a device
    batch, made dense in that order. Returns (data, offsets, caplens) tensors."""
    import torch
    m = order.numel()
    dev = order.device
    if total_bytes is None:
        total_bytes = int(caplens.index_select(0, order.long()).sum(dtype=torch.int64).item()) if m else 0
    out_d = torch.empty(total_bytes + 16, dtype=torch.uint8, device=dev)
    out_o = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    out_c = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    b = _lib.Batch(data.data_ptr(), offsets.data_ptr(), caplens.data_ptr(), offsets.numel(), data.numel())
    sp = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
    _lib.check(_lib.lib().gpk_pack_batch(ctypes.byref(b), order.data_ptr() if m else None, m, out_d.data_ptr(),
                                         out_o.data_ptr(), out_c.data_ptr(), sp))
    return out_d, out_o[:m], out_c[:m]


HELD, EHOLE, EINVALID, EMAXLEN, EPANIC = (_lib.DEFRAG_HELD, _lib.DEFRAG_EHOLE, _lib.DEFRAG_EINVALID,
                                          _lib.DEFRAG_EMAXLEN, _lib.DEFRAG_EPANIC)


class Defragmenter:
    """gpk_defrag_batch (include/gpk_defrag.h): the datagrams
    ip4defrag.DefragIPv4 would have returned for a decoded, DEFRAG-grouped
    batch, every packet's verdict and the fragments still waiting. One call
    behaves like a fresh NewIPv4Defragmenter() fed the batch in order; no
    timeouts (DiscardOlderThan)."""

    def __init__(self, max_packets, device=0):
        self.h = ctypes.c_void_p()
        _lib.check(_lib.lib().gpk_defragger_create(ctypes.byref(self.h), device, int(max_packets)))
        self.max_packets = int(max_packets)

    def defrag(self, data, offsets, caplens, records, layouts, groups, data_cap=None, out_data=None, stream=None):
        """Device tensors in: the batch, its records and layouts, and `groups`
        (Grouper.group(kind=DEFRAG) of it). Returns a dict of device tensors:
        verdict[n], last/length/offsets/caplens/payload_off (n entries, counts[0]
        used), pending (counts[1] used), counts[4] (datagrams, pending, bytes
        needed, overflow) and data. data_cap defaults to the batch's data size,
        which always suffices. {data, offsets[:D], caplens[:D]} is a batch the
        parsers decode; its IPv4.Length is header + payload, while length[j] is
        the reference's out.Length (the payload length, Highest)."""
        import torch
        n = offsets.numel()
        dev = offsets.device
        if out_data is None:
            cap = int(data.numel() if data_cap is None else data_cap)
            out_data = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
        else:
            cap = int(out_data.numel() if data_cap is None else data_cap)
        m = max(n, 1)
        out = dict(verdict=torch.empty(m, dtype=torch.int32, device=dev),
                   last=torch.empty(m, dtype=torch.int32, device=dev),
                   length=torch.empty(m, dtype=torch.int32, device=dev),
                   offsets=torch.empty(m, dtype=torch.int64, device=dev),
                   caplens=torch.empty(m, dtype=torch.int32, device=dev),
                   payload_off=torch.empty(m, dtype=torch.int32, device=dev),
                   pending=torch.empty(m, dtype=torch.int32, device=dev),
                   counts=torch.zeros(4, dtype=torch.int64, device=dev), data=out_data)
        b = _lib.Batch(data.data_ptr(), offsets.data_ptr(), caplens.data_ptr(), n, data.numel())
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        g = _lib.Groups(groups["group_of"].data_ptr(), groups["perm"].data_ptr(), groups["start"].data_ptr(),
                        groups["first"].data_ptr(), groups["counts"].data_ptr())
        d = _lib.Datagrams(out["verdict"].data_ptr(), out["last"].data_ptr(), out["length"].data_ptr(),
                           out["offsets"].data_ptr(), out["caplens"].data_ptr(), out["payload_off"].data_ptr(),
                           out["pending"].data_ptr(), out["counts"].data_ptr(), out_data.data_ptr(), cap)
        sp = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        _lib.check(_lib.lib().gpk_defrag_batch(self.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g),
                                               ctypes.byref(d), sp))
        out["verdict"] = out["verdict"][:n]
        return out

    def close(self):
        if self.h:
            _lib.lib().gpk_defragger_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IPv4Defragmenter:
    """A streaming ip4defrag.IPv4Defragmenter over device batches: the
    fragments still waiting after a batch stay on the device and are put in
    front of the next one (pack_batch of `pending`), which reproduces the
    reference's state. Each call decodes (with layouts), groups and
    reassembles pending + new packets; verdicts and `last` are mapped back to
    the caller's indices (a datagram can only be completed by a new packet).
    No timeouts: flush() is the caller's DiscardOlderThan."""

    def __init__(self, ctx, parser, max_packets, device=0):
        self.ctx, self.parser = ctx, parser
        self.max_packets = int(max_packets)
        self.grouper = Grouper(self.max_packets, device)
        self.defragmenter = Defragmenter(self.max_packets, device)
        self._pending = None  # (data, offsets, caplens) on the device

    @property
    def pending_count(self):
        return 0 if self._pending is None else int(self._pending[1].numel())

    def flush(self):
        """Forget every waiting fragment; returns how many there were."""
        k = self.pending_count
        self._pending = None
        return k

    def defrag(self, data, offsets, caplens):
        """One batch of packets (device tensors: uint8 data, int64 offsets,
        int32 caplens). Returns Defragmenter.defrag's dict for the caller's
        packets, with `verdict` and `last` in the caller's indices and
        counts/pending on the host: datagrams, data, offsets, caplens, ..."""
        import torch
        dev = offsets.device
        P = self.pending_count
        if P:
            pd, po, pc = self._pending
            base = pd.numel()
            data = torch.cat([pd, data])
            offsets = torch.cat([po, offsets + base])
            caplens = torch.cat([pc, caplens])
        n = offsets.numel()
        if n > self.max_packets:
            raise ValueError("pending + batch exceed max_packets")
        if n == 0:
            e32, e64 = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
            return dict(verdict=e32, last=e32, length=e32, offsets=e64, caplens=e32, payload_off=e32, pending=e32,
                        counts=[0, 0, 0, 0], datagrams=0, data=torch.empty(0, dtype=torch.uint8, device=dev))
        rec = torch.zeros(max(n, 1) * 16, dtype=torch.uint8, device=dev)
        lay = torch.zeros(max(n, 1) * 64, dtype=torch.uint8, device=dev)
        flw = torch.zeros(max(n, 1) * 3, dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream()
        self.ctx.decode_device(self.parser, data, offsets, caplens, rec, None, flw, lay, stream=st)
        groups = self.grouper.group(data, offsets, caplens, rec, lay, kind=DEFRAG, stream=st)
        out = self.defragmenter.defrag(data, offsets, caplens, rec, lay, groups, stream=st)
        counts = out["counts"].cpu().tolist()
        D, K = counts[0], counts[1]
        pend = out["pending"][:K]
        if K:
            total = int(caplens.index_select(0, pend.long()).sum(dtype=torch.int64).item())
            d2, o2, c2 = pack_batch(data, offsets, caplens, pend, total_bytes=total, stream=st)
            self._pending = (d2[:total], o2, c2)
        else:
            self._pending = None
        v = out["verdict"][P:]
        out.update(verdict=v, last=out["last"][:D] - P, length=out["length"][:D], offsets=out["offsets"][:D],
                   caplens=out["caplens"][:D], payload_off=out["payload_off"][:D], pending=pend - P,
                   counts=counts, datagrams=D)
        return out

    def close(self):
        self.grouper.close()
        self.defragmenter.close()
