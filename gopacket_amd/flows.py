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
  kind DEFRAG6                             ip6defrag container[fg.Identification]
                                           (ip6defrag/defrag.go:98)

Groups come in order of first appearance; packets inside a group in batch
order. group_of[i] < 0 says why packet i has no key (GROUP_* codes).

  Defragmenter(max_packets).defrag(...)    gpk_defrag_batch (include/gpk_defrag.h):
                                           ip4defrag's reassembly of a DEFRAG-grouped
                                           batch (defrag.go:113-132,214-326)
  IPv4Defragmenter(ctx, parser, n)         the same over a stream of batches; timed=True keeps
                                           LastSeen and gives discard_older_than (:138-149)
  Defragmenter6(max_packets).defrag(...)   gpk_defrag6_batch (include/gpk_defrag6.h):
                                           ip6defrag's reassembly of a DEFRAG6-grouped
                                           batch (ip6defrag/defrag.go:82-178)
  IPv6Defragmenter(ctx, parser, n)         the same over a stream of batches; timed=True keeps
                                           the keys' times and gives discard_older_than (:183-194)
  timestamps_ns(capinfo)                   a CAPINFO_DTYPE array as int64 ns on the device
  Assembler(max_packets).assemble(...)     gpk_tcpasm_batch (include/gpk_tcpasm.h):
                                           tcpassembly's reassembly of a CONNECTION-grouped
                                           batch (assembly.go:536-783, FlushAll :279-290)
  TCPAssembler(ctx, parser, n)             the same over a stream of batches; timed=True keeps
                                           lastSeen and page.Seen and gives flush_older_than
                                           (FlushWithOptions, :238-274)
  Serializer(max_packets).serialize(...)   gpk_serialize_batch (include/gpk_serialize.h):
                                           gopacket.SerializeLayers for a decoded batch, from
                                           its layouts and (edited) fields records
                                           (writer.go:207-218 and the six layers' SerializeTo)
  Detunneler(max_packets).peel(...)        gpk_tunnel_batch (include/gpk_tunnel.h): the GRE,
                                           VXLAN and Geneve headers of the packets whose decode
                                           stopped at one (layers/gre.go, vxlan.go, geneve.go),
                                           and their inner packets as zero-copy batches
  ControlDecoder(max_packets).decode(...)  gpk_control_batch (include/gpk_control.h): the ICMPv4,
                                           ICMPv6 (+Echo) and ARP layers of the packets whose
                                           decode stopped in front of one, and their checksums
  DNSDecoder(max_packets).decode(...)      gpk_dns_batch (include/gpk_dns.h): the DNS messages
                                           of the packets whose decode stopped in front of
                                           LayerTypeDNS: message records, one entry per question
                                           or resource record, and the decompressed names
  TLSDecoder(max_packets).decode(...)      gpk_tls_batch (include/gpk_tls.h): the TLS messages
                                           of the packets whose decode stopped in front of
                                           LayerTypeTLS: message records, one entry per TLS
                                           record and per ClientHello, and the server names
  TLSStreamDecoder(max_streams).decode(...) gpk_tls_streams (include/gpk_tls_streams.h): the TLS
                                           records of the streams Assembler.assemble laid out:
                                           record boundaries, the unfinished tail, one entry per
                                           record and per ClientHello, and the server names
  TLSStreams(ctx, parser, n)               the same over a stream of batches, on a TCPAssembler
  DNSStreamDecoder(max_streams, max_msgs).decode(...)
                                           gpk_dns_streams (include/gpk_dns_streams.h): the DNS
                                           messages of the streams Assembler.assemble laid out:
                                           message boundaries by the two length bytes, the
                                           unfinished tail, one entry per message, its questions
                                           and records, and the decompressed names
  DNSStreams(ctx, parser, n)               the same over a stream of batches, on a TCPAssembler
"""
import ctypes

from . import _lib

CONNECTION, DEFRAG, NET_BUCKET, DEFRAG6 = (_lib.GROUP_CONNECTION, _lib.GROUP_DEFRAG, _lib.GROUP_NET_BUCKET,
                                           _lib.GROUP_DEFRAG6)
NONE, USELESS, FRAG_TOO_SMALL, FRAG_OFFSET, FRAG_OVERRUN, UNKNOWN = (
    _lib.GROUP_NONE, _lib.GROUP_USELESS, _lib.GROUP_FRAG_TOO_SMALL, _lib.GROUP_FRAG_OFFSET,
    _lib.GROUP_FRAG_OVERRUN, _lib.GROUP_UNKNOWN)


class _Handle:
    """Owns a handle of the C ABI: made by the entry `_create`(&h, device,
    max_packets), released by the entry `_destroy`(h)."""
    _create = _destroy = None

    def __init__(self, max_packets, device=0):
        self.h = ctypes.c_void_p()
        _lib.check(getattr(_lib.lib(), self._create)(ctypes.byref(self.h), device, int(max_packets)))
        self.max_packets = int(max_packets)

    def close(self):
        if self.h:
            getattr(_lib.lib(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _out_buffer(data, data_cap, out_data, dev):
    """-> (out_data, cap): the caller's output bytes, or ones of data_cap (default: the batch's size) + 16 spare."""
    import torch
    if out_data is None:
        cap = int(data.numel() if data_cap is None else data_cap)
        return torch.empty(cap + 16, dtype=torch.uint8, device=dev), cap
    return out_data, int(out_data.numel() if data_cap is None else data_cap)


class Grouper(_Handle):
    _create, _destroy = "gpk_grouper_create", "gpk_grouper_destroy"

    @staticmethod
    def _outputs(offsets):
        import torch
        n, dev = offsets.numel(), offsets.device
        return dict(group_of=torch.empty(n, dtype=torch.int32, device=dev),
                    perm=torch.empty(n, dtype=torch.int32, device=dev),
                    start=torch.empty(n + 1, dtype=torch.int32, device=dev),
                    first=torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                    counts=torch.zeros(2, dtype=torch.int32, device=dev))

    def group(self, data, offsets, caplens, records, layouts=None, flows=None, kind=CONNECTION, buckets=8,
              out=None, stream=None):
        """Device tensors in (torch, as gpk_decode_batch takes them); returns
        dict(group_of, perm, start, first, counts) of device tensors (or fills `out`)."""
        if out is None:
            out = self._outputs(offsets)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, flows.data_ptr() if flows is not None else None,
                         layouts.data_ptr() if layouts is not None else None)
        g = _lib.Groups.of(out)
        _lib.check(_lib.lib().gpk_group_batch(self.h, ctypes.byref(b), ctypes.byref(r), int(kind), int(buckets),
                                              ctypes.byref(g), _lib.stream_ptr(stream)))
        return out

    def decode_group(self, ctx, parser, data, offsets, caplens, records, err_args=None, flows=None, kind=CONNECTION,
                     out=None, stream=None):
        """gpk_decode_group_batch: decode (records/err_args/flows as
        Context.decode_device, no layouts) and group by `kind` (CONNECTION or
        DEFRAG) with the key derived inside the decode kernel."""
        if out is None:
            out = self._outputs(offsets)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), err_args.data_ptr() if err_args is not None else None,
                         flows.data_ptr() if flows is not None else None, None)
        g = _lib.Groups.of(out)
        _lib.check(_lib.lib().gpk_decode_group_batch(ctx.h, parser.h, ctypes.byref(b), ctypes.byref(r), self.h,
                                                     int(kind), ctypes.byref(g), _lib.stream_ptr(stream)))
        return out

    def hashes(self, n):
        """gpk_grouper_hashes (a test aid): the 64-bit key hashes of the first n
        packets of the last call, as a numpy uint64 array; unspecified where a
        packet has no key. Synchronises the device."""
        import numpy as np
        out = np.zeros(int(n), np.uint64)
        _lib.check(_lib.lib().gpk_grouper_hashes(self.h, int(n), out.ctypes.data))
        return out

    @staticmethod
    def to_lists(out):
        """Host view: (groups: list of packet-index lists in group order, group_of list)."""
        counts = out["counts"].cpu().tolist()
        G, K = counts[0], counts[1]
        perm = out["perm"][:K].cpu().tolist()
        start = out["start"][:G + 1].cpu().tolist()
        return [perm[start[g]:start[g + 1]] for g in range(G)], out["group_of"].cpu().tolist()


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
    b = _lib.Batch.of(data, offsets, caplens)
    sp = _lib.stream_ptr(stream)
    _lib.check(_lib.lib().gpk_pack_batch(ctypes.byref(b), order.data_ptr() if m else None, m, out_d.data_ptr(),
                                         out_o.data_ptr(), out_c.data_ptr(), sp))
    return out_d, out_o[:m], out_c[:m]


def timestamps_ns(capinfo, device=None):
    """The capture timestamps of a _lib.CAPINFO_DTYPE array (a capture reader's
    or replay's per-packet info) as time.Time.UnixNano(): an int64 device
    tensor of ts_sec * 10^9 + ts_nsec, what the timed reassemblers take."""
    import numpy as np
    import torch
    ci = np.asarray(capinfo)
    ns = ci["ts_sec"].astype(np.int64) * 1000000000 + ci["ts_nsec"].astype(np.int64)
    return torch.from_numpy(np.ascontiguousarray(ns)).to("cuda" if device is None else device)


def _time_arg(n, dev, seen, discard_older_than):
    """-> (DefragTime, pending_seen, time_counts) for a timed defrag call."""
    import torch
    if seen.dtype != torch.int64 or seen.numel() != n:
        raise ValueError("seen: one int64 timestamp per packet")
    seen = seen.contiguous()
    ps = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    tc = torch.zeros(2, dtype=torch.int64, device=dev)
    t = _lib.DefragTime(seen.data_ptr() if n else None, 0 if discard_older_than is None else 1,
                        0 if discard_older_than is None else int(discard_older_than), ps.data_ptr(), tc.data_ptr())
    return t, ps, tc, seen


HELD, EHOLE, EINVALID, EMAXLEN, EPANIC = (_lib.DEFRAG_HELD, _lib.DEFRAG_EHOLE, _lib.DEFRAG_EINVALID,
                                          _lib.DEFRAG_EMAXLEN, _lib.DEFRAG_EPANIC)


class Defragmenter(_Handle):
    """gpk_defrag_batch (include/gpk_defrag.h): the datagrams
    ip4defrag.DefragIPv4 would have returned for a decoded, DEFRAG-grouped
    batch, every packet's verdict and the fragments still waiting. One call
    behaves like a fresh NewIPv4Defragmenter() fed the batch in order. With
    `seen` (gpk_defrag_batch_timed) the keys keep LastSeen and
    DiscardOlderThan can run after the batch."""

    _create, _destroy = "gpk_defragger_create", "gpk_defragger_destroy"

    def defrag(self, data, offsets, caplens, records, layouts, groups, data_cap=None, out_data=None, stream=None,
               seen=None, discard_older_than=None):
        """Device tensors in: the batch, its records and layouts, and `groups`
        (Grouper.group(kind=DEFRAG) of it). seen: int64 ns per packet
        (DefragIPv4WithTimestamp's t; for a carried fragment its key's LastSeen);
        with it the result also has pending_seen (LastSeen of pending[k]'s key)
        and time_counts[2] (keys discarded, packets dropped), and
        discard_older_than=t runs DiscardOlderThan(t) after the batch: pending and
        counts[1] are the survivors. Returns a dict of device tensors:
        verdict[n], last/length/offsets/caplens/payload_off (n entries, counts[0]
        used), pending (counts[1] used), counts[4] (datagrams, pending, bytes
        needed, overflow) and data. data_cap defaults to the batch's data size,
        which always suffices. {data, offsets[:D], caplens[:D]} is a batch the
        parsers decode; its IPv4.Length is header + payload, while length[j] is
        the reference's out.Length (the payload length, Highest)."""
        import torch
        n = offsets.numel()
        dev = offsets.device
        out_data, cap = _out_buffer(data, data_cap, out_data, dev)
        m = max(n, 1)
        out = dict(verdict=torch.empty(m, dtype=torch.int32, device=dev),
                   last=torch.empty(m, dtype=torch.int32, device=dev),
                   length=torch.empty(m, dtype=torch.int32, device=dev),
                   offsets=torch.empty(m, dtype=torch.int64, device=dev),
                   caplens=torch.empty(m, dtype=torch.int32, device=dev),
                   payload_off=torch.empty(m, dtype=torch.int32, device=dev),
                   pending=torch.empty(m, dtype=torch.int32, device=dev),
                   counts=torch.zeros(4, dtype=torch.int64, device=dev), data=out_data)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        g = _lib.Groups.of(groups)
        d = _lib.Datagrams(out["verdict"].data_ptr(), out["last"].data_ptr(), out["length"].data_ptr(),
                           out["offsets"].data_ptr(), out["caplens"].data_ptr(), out["payload_off"].data_ptr(),
                           out["pending"].data_ptr(), out["counts"].data_ptr(), out_data.data_ptr(), cap)
        sp = _lib.stream_ptr(stream)
        if seen is None:
            if discard_older_than is not None:
                raise ValueError("discard_older_than needs seen")
            _lib.check(_lib.lib().gpk_defrag_batch(self.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g),
                                                   ctypes.byref(d), sp))
        else:
            t, out["pending_seen"], out["time_counts"], seen = _time_arg(n, dev, seen, discard_older_than)
            _lib.check(_lib.lib().gpk_defrag_batch_timed(self.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g),
                                                         ctypes.byref(d), ctypes.byref(t), sp))
        out["verdict"] = out["verdict"][:n]
        return out


def _prepend(carried, data, offsets, caplens, spare=0):
    """The carried packets (data, offsets, caplens) put in front of a batch,
    with `spare` zero bytes behind the data."""
    import torch
    pd, po, pc = carried
    tail = [torch.zeros(spare, dtype=torch.uint8, device=offsets.device)] if spare else []
    return torch.cat([pd, data] + tail), torch.cat([po, offsets + pd.numel()]), torch.cat([pc, caplens])


def _decode_group(ctx, parser, grouper, data, offsets, caplens, kind):
    """Decode a batch (with layouts) and group it by `kind` on the current
    stream -> (records, layouts, groups, stream)."""
    import torch
    n, dev = offsets.numel(), offsets.device
    rec = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    lay = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    flw = torch.zeros(n * 3, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream()
    ctx.decode_device(parser, data, offsets, caplens, rec, None, flw, lay, stream=st)
    return rec, lay, grouper.group(data, offsets, caplens, rec, lay, kind=kind, stream=st), st


def _pack_carry(data, offsets, caplens, order, stream):
    """pack_batch of the packets that go into the next call, cut to their bytes."""
    import torch
    total = int(caplens.index_select(0, order.long()).sum(dtype=torch.int64).item())
    d2, o2, c2 = pack_batch(data, offsets, caplens, order, total_bytes=total, stream=stream)
    return d2[:total], o2, c2


class _StreamingDefragmenter:
    """What IPv4Defragmenter and IPv6Defragmenter share: the fragments kept on
    the device between calls, and a step that puts them in front of the batch,
    decodes, groups, reassembles, packs what is still pending and maps the
    results back to the caller's indices. A subclass gives the grouping kind,
    the batch reassembler, the per-datagram keys, the reassembly call and, if
    it has one, a filter on what stays pending."""
    _kind = _reassembler = None
    _per_datagram = ()  # the result's arrays with one entry per datagram; last and head are packet indices

    def __init__(self, ctx, parser, max_packets, device=0, timed=False):
        self.ctx, self.parser = ctx, parser
        self.max_packets = int(max_packets)
        self.timed = bool(timed)
        self.grouper = Grouper(self.max_packets, device)
        self.defragmenter = self._reassembler(self.max_packets, device)
        self._pending = None  # (data, offsets, caplens) on the device
        self._pending_seen = None  # timed: int64[pending], the time (IPv4: LastSeen) of each carried fragment's key

    @property
    def pending_count(self):
        return 0 if self._pending is None else int(self._pending[1].numel())

    def flush(self):
        """Forget every waiting (held) fragment; returns how many there were."""
        k = self.pending_count
        self._pending = self._pending_seen = None
        return k

    def discard_older_than(self, t):
        """DiscardOlderThan(t), t in int64 ns: the keys whose LastSeen < t (IPv6:
        whose last call was before t) are forgotten with their fragments. Returns
        the number of keys discarded (the reference's return value). timed=True
        only."""
        import torch
        if not self.timed:
            raise NotImplementedError("discard_older_than: time is out of scope unless timed=True")
        if not self.pending_count:
            return 0
        dev = self._pending[1].device
        out = self._step(torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                         torch.empty(0, dtype=torch.int32, device=dev),
                         torch.empty(0, dtype=torch.int64, device=dev), int(t))
        return out["time_counts"][0]

    def defrag(self, data, offsets, caplens, timestamps=None):
        """One batch of packets (device tensors: uint8 data, int64 offsets,
        int32 caplens; timed: int64 ns timestamps, one per packet). Returns
        the batch reassembler's dict (Defragmenter.defrag's, Defragmenter6.defrag's)
        for the caller's packets, with `verdict`, `last` (and IPv6's `head`) in
        the caller's indices and counts/pending on the host: datagrams, data,
        offsets, caplens, ..."""
        if self.timed != (timestamps is not None):
            raise ValueError("timestamps go with timed=True, and only with it")
        return self._step(data, offsets, caplens, timestamps, None)

    def _reassemble(self, batch, groups, carried, stream, timed_args):
        """-> (the reassembler's result, its counts on the host)"""
        raise NotImplementedError

    def _keep_pending(self, out, groups, pend, datagrams):
        """A bool mask over `pend` of what stays pending, or None for all of it."""
        return None

    def _step(self, data, offsets, caplens, timestamps, discard_t):
        import torch
        dev = offsets.device
        P = self.pending_count
        if P:
            data, offsets, caplens = _prepend(self._pending, data, offsets, caplens)
            if self.timed:
                timestamps = torch.cat([self._pending_seen, timestamps])
        n = offsets.numel()
        if n > self.max_packets:
            raise ValueError("pending + batch exceed max_packets")
        if n == 0:
            e32, e64 = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
            return dict(verdict=e32, **{k: e64 if k == "offsets" else e32 for k in self._per_datagram}, pending=e32,
                        counts=[0, 0, 0, 0], datagrams=0, data=torch.empty(0, dtype=torch.uint8, device=dev),
                        **(dict(pending_seen=e64, time_counts=[0, 0]) if self.timed else {}))
        rec, lay, groups, st = _decode_group(self.ctx, self.parser, self.grouper, data, offsets, caplens, self._kind)
        tk = dict(seen=timestamps, discard_older_than=discard_t) if self.timed else {}
        out, counts = self._reassemble((data, offsets, caplens, rec, lay), groups, P, st, tk)
        D, K = counts[0], counts[1]
        pend = out["pending"][:K]
        pseen = out["pending_seen"][:K] if self.timed else None
        keep = self._keep_pending(out, groups, pend, D) if K and D else None
        if keep is not None:
            pend = pend[keep]
            if self.timed:
                pseen = pseen[keep]
            K = counts[1] = int(pend.numel())
        self._pending = _pack_carry(data, offsets, caplens, pend.contiguous(), st) if K else None
        if self.timed:
            self._pending_seen = pseen.clone() if K else None
            out.update(pending_seen=pseen, time_counts=out["time_counts"].cpu().tolist())
        per = {k: out[k][:D] - P if k in ("last", "head") else out[k][:D] for k in self._per_datagram}
        out.update(verdict=out["verdict"][P:], **per, pending=pend - P, counts=counts, datagrams=D)
        return out

    def close(self):
        self.grouper.close()
        self.defragmenter.close()


class IPv4Defragmenter(_StreamingDefragmenter):
    """A streaming ip4defrag.IPv4Defragmenter over device batches: the
    fragments still waiting after a batch stay on the device and are put in
    front of the next one (pack_batch of `pending`), which reproduces the
    reference's state. Each call decodes (with layouts), groups and
    reassembles pending + new packets; verdicts and `last` are mapped back to
    the caller's indices (a datagram can only be completed by a new packet).

    timed=False keeps no time: flush() is then the caller's only
    DiscardOlderThan. timed=True: defrag() takes the packets' timestamps
    (int64 ns, greater than INT64_MIN), every key keeps its LastSeen on the
    device beside its fragments, and discard_older_than(t) is
    DiscardOlderThan(t)."""

    _kind, _reassembler = DEFRAG, Defragmenter
    _per_datagram = ("last", "length", "offsets", "caplens", "payload_off")

    def _reassemble(self, batch, groups, carried, stream, timed_args):
        out = self.defragmenter.defrag(*batch, groups, stream=stream, **timed_args)
        return out, out["counts"].cpu().tolist()


HELD6, CARRIED6 = _lib.DEFRAG6_HELD, _lib.DEFRAG6_CARRIED


class Defragmenter6(_Handle):
    """gpk_defrag6_batch (include/gpk_defrag6.h): the IPv6 layers
    ip6defrag.DefragIPv6 would have returned for a decoded, DEFRAG6-grouped
    batch, every packet's verdict and the fragments it holds. One call behaves
    like a fresh NewIPv6Defragmenter() fed the batch in order. A key is never
    flushed (a completed datagram comes again with every later call on its
    key). With `seen` (gpk_defrag6_batch_timed) the keys keep their time and
    DiscardOlderThan can run after the batch."""

    _create, _destroy = "gpk_defragger6_create", "gpk_defragger6_destroy"

    def defrag(self, data, offsets, caplens, records, layouts, groups, carry=0, data_cap=None, out_data=None,
               stream=None, seen=None, discard_older_than=None):
        """Device tensors in: the batch, its records and layouts, and `groups`
        (Grouper.group(kind=DEFRAG6) of it). The calls of the first `carry`
        packets build state only (verdict CARRIED6, nothing emitted). seen: int64
        ns per packet (the call's time; for a carry packet its key's time); with
        it the result also has pending_seen (the time of pending[k]'s key) and
        time_counts[2] (keys discarded, listed fragments dropped), and
        discard_older_than=t runs DiscardOlderThan(t) after the batch: pending and
        counts[1] are the survivors. Returns a
        dict of device tensors: verdict[n], last/head/length/offsets/caplens/
        payload_off (n entries, counts[0] used), pending (counts[1] used),
        counts[4] (datagrams, pending, bytes needed, overflow) and data.
        data_cap defaults to the batch's data size, which does NOT always
        suffice here: every later call on a completed key returns its datagram
        again. On overflow (counts[3]) the datagrams that fit are whole and
        counts[2] is the capacity a second call needs. {data, offsets[:D],
        caplens[:D]} is a batch the parsers decode; length[j] is the payload's
        byte count (the reference's own Length field stays 0)."""
        import torch
        n = offsets.numel()
        dev = offsets.device
        out_data, cap = _out_buffer(data, data_cap, out_data, dev)
        m = max(n, 1)
        i32 = torch.int32
        out = dict(verdict=torch.empty(m, dtype=i32, device=dev), last=torch.empty(m, dtype=i32, device=dev),
                   head=torch.empty(m, dtype=i32, device=dev), length=torch.empty(m, dtype=i32, device=dev),
                   offsets=torch.empty(m, dtype=torch.int64, device=dev),
                   caplens=torch.empty(m, dtype=i32, device=dev), payload_off=torch.empty(m, dtype=i32, device=dev),
                   pending=torch.empty(m, dtype=i32, device=dev),
                   counts=torch.zeros(4, dtype=torch.int64, device=dev), data=out_data)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        g = _lib.Groups.of(groups)
        d = _lib.Datagrams6(*[out[k].data_ptr() for k in ("verdict", "last", "head", "length", "offsets", "caplens",
                                                          "payload_off", "pending", "counts")],
                            out_data.data_ptr(), cap)
        sp = _lib.stream_ptr(stream)
        if seen is None:
            if discard_older_than is not None:
                raise ValueError("discard_older_than needs seen")
            _lib.check(_lib.lib().gpk_defrag6_batch(self.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g),
                                                    int(carry), ctypes.byref(d), sp))
        else:
            t, out["pending_seen"], out["time_counts"], seen = _time_arg(n, dev, seen, discard_older_than)
            _lib.check(_lib.lib().gpk_defrag6_batch_timed(self.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g),
                                                          int(carry), ctypes.byref(d), ctypes.byref(t), sp))
        out["verdict"] = out["verdict"][:n]
        return out


class IPv6Defragmenter(_StreamingDefragmenter):
    """A streaming ip6defrag.IPv6Defragmenter over device batches: the listed
    fragments stay on the device (pack_batch of `pending`) and go in front of
    the next batch as its `carry` packets, which reproduces the reference's
    lists exactly (first arrivals stay first, nothing was ever removed) without
    returning their datagrams a second time. Each call decodes (with layouts),
    groups and reassembles carried + new packets; `verdict`, `last` and `head`
    are mapped back to the caller's indices. head[j] < 0 says the header came
    from a carried packet of an earlier batch (-1 is the last of them); its
    bytes are in the datagram all the same.

    The reference never removes a key (only DiscardOlderThan does), so by
    default the state grows without bound, as the reference's does when
    DiscardOlderThan is never called. timed=False keeps no time: flush() is
    then the caller's only DiscardOlderThan. timed=True: defrag() takes the
    packets' timestamps (int64 ns; they play the reference's time.Now()),
    every key keeps the time of its last call on the device beside its
    fragments, and discard_older_than(t) is DiscardOlderThan(t). Scope decision
    that departs from the reference: with drop_completed=True a key that
    returned a datagram in a call is not carried into the next one, so it does
    not return that datagram again in later batches and its state is freed."""

    _kind, _reassembler = DEFRAG6, Defragmenter6
    _per_datagram = ("last", "head", "length", "offsets", "caplens", "payload_off")

    def __init__(self, ctx, parser, max_packets, device=0, drop_completed=False, timed=False):
        super().__init__(ctx, parser, max_packets, device, timed)
        self.drop_completed = bool(drop_completed)

    def _reassemble(self, batch, groups, carried, stream, timed_args):
        out = self.defragmenter.defrag(*batch, groups, carry=carried, stream=stream, **timed_args)
        counts = out["counts"].cpu().tolist()
        if counts[3]:  # re-emission: the batch's size does not bound the datagrams' bytes
            out = self.defragmenter.defrag(*batch, groups, carry=carried, data_cap=counts[2], stream=stream,
                                           **timed_args)
            counts = out["counts"].cpu().tolist()
        return out, counts

    def _keep_pending(self, out, groups, pend, datagrams):
        import torch
        if not self.drop_completed:
            return None
        gof = groups["group_of"].long()
        done = torch.zeros(gof.numel(), dtype=torch.bool, device=gof.device)
        done[gof.index_select(0, out["last"][:datagrams].long())] = True
        return ~done.index_select(0, gof.index_select(0, pend.long()))


DIRECT, QUEUED, NOCONN, CARRIED, EBADCARRY, TCP_EPANIC = (
    _lib.TCPASM_DIRECT, _lib.TCPASM_QUEUED, _lib.TCPASM_NOCONN, _lib.TCPASM_CARRIED, _lib.TCPASM_EBADCARRY,
    _lib.TCPASM_EPANIC)


class Assembler(_Handle):
    """gpk_tcpasm_batch (include/gpk_tcpasm.h): the Reassembly objects
    tcpassembly's Assembler would have handed every stream of a decoded,
    CONNECTION-grouped batch, the streams' bytes, every packet's verdict and
    the state at the end. One call behaves like a fresh NewAssembler with
    MaxBufferedPagesPerConnection = max_pages fed the batch in order, then
    FlushAll() if `flush`. With `seen` (gpk_tcpasm_batch_timed) the connections
    keep lastSeen and FlushWithOptions{T} can run after the batch."""

    _create, _destroy = "gpk_tcpasm_create", "gpk_tcpasm_destroy"

    def assemble(self, data, offsets, caplens, records, layouts, groups, max_pages=0, flush=False, data_cap=None,
                 stream=None, chunk_cap=None, out_data=None, carry_code=None, carry_seq=None, seen=None,
                 flush_older=0, t=0):
        """Device tensors in: the batch, its records and layouts, and `groups`
        (Grouper.group(kind=CONNECTION) of it). Returns a dict of device tensors:
        verdict[n], stream_of[n], chunks (uint8 view of gpk_tcp_chunk[chunk_cap],
        _lib.TCP_CHUNK_DTYPE on the host), stream_group/first/closed[n],
        stream_chunk0/stream_data0[n+1], conn_seq/conn_stream[n] (per group),
        pend_pkt/pend_page[chunk_cap], counts[8] and data. chunk_cap defaults to
        n + data bytes / 1900 and data_cap to the batch's data size, which always
        suffice. carry_code (int32 bit patterns) / carry_seq (int64): the first
        carry_code.numel() packets are carried entries. seen: int64 ns per
        packet (for a CARRY_CONN entry the connection's lastSeen, for a
        CARRY_PAGE entry the page's Seen); with it the result also has
        conn_last_seen[n] (per group) and time_counts[2] (flushed, closed), and
        flush_older = 1 (FlushWithOptions{T: t}) or 2 (CloseAll too:
        FlushOlderThan(t)) runs after the batch."""
        import torch
        n = offsets.numel()
        dev = offsets.device
        out_data, cap = _out_buffer(data, data_cap, out_data, dev)
        ccap = int(n + data.numel() // _lib.TCPASM_PAGE_BYTES if chunk_cap is None else chunk_cap)
        m, cm = max(n, 1), max(ccap, 1)
        i32, i64 = torch.int32, torch.int64
        out = dict(verdict=torch.empty(m, dtype=i32, device=dev), stream_of=torch.empty(m, dtype=i32, device=dev),
                   chunks=torch.empty(cm * 40, dtype=torch.uint8, device=dev),
                   stream_group=torch.empty(m, dtype=i32, device=dev),
                   stream_first=torch.empty(m, dtype=i32, device=dev),
                   stream_closed=torch.empty(m, dtype=i32, device=dev),
                   stream_chunk0=torch.empty(m + 1, dtype=i32, device=dev),
                   stream_data0=torch.empty(m + 1, dtype=i64, device=dev),
                   conn_seq=torch.empty(m, dtype=i64, device=dev), conn_stream=torch.empty(m, dtype=i32, device=dev),
                   pend_pkt=torch.empty(cm, dtype=i32, device=dev), pend_page=torch.empty(cm, dtype=i32, device=dev),
                   counts=torch.zeros(8, dtype=i64, device=dev), data=out_data)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        g = _lib.Groups.of(groups)
        carried = 0 if carry_code is None else int(carry_code.numel())
        op = _lib.TcpasmOpts(int(max_pages), 1 if flush else 0, carried,
                             carry_code.data_ptr() if carried else None, carry_seq.data_ptr() if carried else None)
        o = _lib.TcpStreams(*[out[k].data_ptr() for k in (
            "verdict", "stream_of", "chunks", "stream_group", "stream_first", "stream_closed", "stream_chunk0",
            "stream_data0", "conn_seq", "conn_stream", "pend_pkt", "pend_page", "counts")], out_data.data_ptr(), ccap,
            cap)
        sp = _lib.stream_ptr(stream)
        if seen is None:
            if flush_older:
                raise ValueError("flush_older needs seen")
            _lib.check(_lib.lib().gpk_tcpasm_batch(self.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g),
                                                   ctypes.byref(op), ctypes.byref(o), sp))
        else:
            if seen.dtype != i64 or seen.numel() != n:
                raise ValueError("seen: one int64 timestamp per packet")
            seen = seen.contiguous()
            out["conn_last_seen"] = torch.empty(m, dtype=i64, device=dev)
            out["time_counts"] = torch.zeros(2, dtype=i64, device=dev)
            tm = _lib.TcpasmTime(seen.data_ptr() if n else None, int(flush_older), int(t),
                                 out["conn_last_seen"].data_ptr(), out["time_counts"].data_ptr())
            _lib.check(_lib.lib().gpk_tcpasm_batch_timed(self.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(g),
                                                         ctypes.byref(op), ctypes.byref(o), ctypes.byref(tm), sp))
        out["verdict"], out["stream_of"] = out["verdict"][:n], out["stream_of"][:n]
        return out


class TCPAssembler:
    """A streaming tcpassembly.Assembler over device batches. The open
    connections and the pages still listed after a batch stay on the device
    (pack_batch of their packets) and go in front of the next batch as carried
    entries, which reproduces the reference's state. Stream ids are global over
    the calls; a source packet or call is (batch number, index), batch numbers
    counting assemble() calls from 0. max_packets bounds carried entries plus
    batch; the workspaces are rebuilt larger when open connections outgrow it.

    timed=False keeps no time: flush_all() is FlushAll(), nothing ages out.
    timed=True: assemble() takes the packets' timestamps (int64 ns, greater than
    INT64_MIN), every connection keeps its lastSeen and every listed page its
    Seen on the device beside the carried entries, every chunk carries `seen`
    (Reassembly.Seen), and flush_older_than(t) is FlushOlderThan(t). A new
    connection starts with no lastSeen; the reference lets it inherit a closed
    connection's through its free list (include/gpk_tcpasm.h)."""

    def __init__(self, ctx, parser, max_packets, max_pages=0, device=0, keys=False, timed=False):
        self.timed = bool(timed)
        self._carry_seen = None  # timed: int64 per carried entry (lastSeen of a CARRY_CONN, Seen of a CARRY_PAGE)
        self.ctx, self.parser = ctx, parser
        self.max_packets, self.max_pages = int(max_packets), int(max_pages)
        self.keys = keys  # also return every new stream's key (its flows' bytes)
        self.device = device
        self.grouper = Grouper(self.max_packets, device)
        self.assembler = Assembler(self.max_packets, device)
        self._carry = None  # (data, offsets, caplens, code[], seq[], gid[], origin[(batch, index)])
        self._streams = 0   # global ids handed out so far
        self._batch = 0
        self._last = None   # the device arrays of the last call that had packets

    @property
    def open_count(self):
        return 0 if self._carry is None else sum(1 for c in self._carry[3] if c & _lib.TCPASM_CARRY_CONN)

    def flush_all(self):
        """FlushAll(): a carried-only call with flush. Returns assemble()'s result."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if self._carry is None else self._carry[1].device
        e = torch.empty(0, dtype=torch.uint8, device=dev)
        return self._run(e, torch.empty(0, dtype=torch.int64, device=dev),
                         torch.empty(0, dtype=torch.int32, device=dev), True, False,
                         torch.empty(0, dtype=torch.int64, device=dev) if self.timed else None)

    def flush_older_than(self, t, close_all=True):
        """FlushWithOptions(FlushOptions{T: t, CloseAll: close_all}); with
        close_all FlushOlderThan(t). t in int64 ns. A carried-only call: returns
        assemble()'s result plus flushed and closed, the reference's two return
        values; a flush call is ("flush", round). timed=True only."""
        import torch
        if not self.timed:
            raise NotImplementedError("flush_older_than: time is out of scope unless timed=True")
        dev = torch.device("cuda", torch.cuda.current_device()) if self._carry is None else self._carry[1].device
        e = torch.empty(0, dtype=torch.uint8, device=dev)
        return self._run(e, torch.empty(0, dtype=torch.int64, device=dev),
                         torch.empty(0, dtype=torch.int32, device=dev), False, False,
                         torch.empty(0, dtype=torch.int64, device=dev), 2 if close_all else 1, int(t))

    def assemble(self, data, offsets, caplens, timestamps=None):
        """One batch (device tensors: uint8 data, int64 offsets, int32 caplens;
        timed: int64 ns timestamps, one per packet).
        Returns dict(verdict, stream_of (global ids, per caller's packet),
        streams: [dict(id, new, closed, chunks: [dict(src, src_off, len, skip,
        call, flags, dst)], data0, data1)], data (device), counts). src and call
        are (batch, index); a flush call is ("flush", round). With keys=True a
        new stream also has key = (net type 4 or 6, src, dst, sport, dport) as
        bytes, from its creating packet."""
        if self.timed != (timestamps is not None):
            raise ValueError("timestamps go with timed=True, and only with it")
        return self._run(data, offsets, caplens, False, True, timestamps)

    def _run(self, data, offsets, caplens, flush, count_batch, timestamps=None, flush_older=0, t=0):
        import numpy as np
        import torch
        dev = offsets.device
        P = 0 if self._carry is None else len(self._carry[3])
        code = seq = None
        if P:
            ccode, cseq, cgid, corigin = self._carry[3:]
            # 16 spare bytes: the byte mover's aligned loads may reach past the last payload
            data, offsets, caplens = _prepend(self._carry[:3], data, offsets, caplens, spare=16)
            code = torch.tensor(np.array(ccode, dtype=np.uint32).view(np.int32), dtype=torch.int32, device=dev)
            seq = torch.tensor(cseq, dtype=torch.int64, device=dev)
            if self.timed:
                timestamps = torch.cat([torch.tensor(self._carry_seen, dtype=torch.int64, device=dev), timestamps])
        else:
            cgid, corigin = [], []
        n = offsets.numel()
        if n > self.max_packets:  # open connections accumulate: the workspaces grow with them
            self.close()
            self.max_packets = max(n, 2 * self.max_packets)
            self.grouper = Grouper(self.max_packets, self.device)
            self.assembler = Assembler(self.max_packets, self.device)
        bno = self._batch
        if count_batch:
            self._batch += 1
        self._last = None
        if n == 0:
            return dict(verdict=[], stream_of=[], streams=[], data=torch.empty(0, dtype=torch.uint8, device=dev),
                        counts=[0] * 8, **(dict(flushed=0, closed=0) if self.timed else {}))
        rec, lay, groups, st = _decode_group(self.ctx, self.parser, self.grouper, data, offsets, caplens, CONNECTION)
        out = self.assembler.assemble(data, offsets, caplens, rec, lay, groups, max_pages=self.max_pages, flush=flush,
                                      stream=st, carry_code=code, carry_seq=seq,
                                      **(dict(seen=timestamps, flush_older=flush_older, t=t) if self.timed else {}))
        counts = out["counts"].cpu().tolist()
        seen = timestamps.cpu().tolist() if self.timed else None
        S, C, NP = counts[0], counts[1], counts[3]
        G = int(groups["counts"][0].item())
        chunks = out["chunks"].cpu().numpy().view(_lib.TCP_CHUNK_DTYPE)[:C]
        first = out["stream_first"][:S].cpu().tolist()
        closed = out["stream_closed"][:S].cpu().numpy().view(np.uint32).tolist()
        chunk0 = out["stream_chunk0"][:S + 1].cpu().tolist()
        data0 = out["stream_data0"][:S + 1].cpu().tolist()

        def origin(i):
            return corigin[i] if i < P else (bno, i - P)

        def call(c):
            return ("flush", c & 0x7FFFFFFF) if c & _lib.TCPASM_CALL_FLUSH else origin(c)

        ids, streams = [], []
        for j in range(S):
            new = first[j] >= P
            if new:
                ids.append(self._streams)
                self._streams += 1
            else:
                ids.append(cgid[first[j]])
            ch = [dict(src=origin(int(c["src"])), src_off=int(c["src_off"]), len=int(c["len"]), skip=int(c["skip"]),
                       call=call(int(c["call"])), flags=int(c["flags"]), dst=int(c["dst"]))
                  for c in chunks[chunk0[j]:chunk0[j + 1]]]
            if self.timed:  # Reassembly.Seen: the source packet's timestamp
                for d, c in zip(ch, chunks[chunk0[j]:chunk0[j + 1]]):
                    d["seen"] = seen[int(c["src"])]
            streams.append(dict(id=ids[j], new=new, first=origin(first[j]), closed=None if closed[j] == _lib.TCPASM_OPEN else call(closed[j]),
                                chunks=ch, data0=data0[j], data1=data0[j + 1]))
        if self.keys:
            new = [j for j in range(S) if streams[j]["new"]]
            if new:
                fi = torch.tensor([first[j] for j in new], dtype=torch.int32, device=dev)
                hd, ho, _ = pack_batch(data, offsets, caplens, fi, stream=st)
                hd, ho = hd.cpu().numpy(), ho.cpu().tolist()
                starts = lay.view(torch.int32).view(n, 16).index_select(0, fi.long())[:, :8].cpu().tolist()
                for j, at, ls in zip(new, ho, starts):
                    ip4, ip6, tcp = ls[2], ls[3], ls[5]  # gpk_layout slots; -1 = absent
                    six = ip6 >= 0 and ip6 < tcp and not (ip4 >= 0 and ip6 < ip4 < tcp)
                    a = at + (ip6 + 8 if six else ip4 + 12)
                    w = 16 if six else 4
                    t = at + tcp
                    streams[j]["key"] = (6 if six else 4, hd[a:a + w].tobytes(), hd[a + w:a + 2 * w].tobytes(),
                                         hd[t:t + 2].tobytes(), hd[t + 2:t + 4].tobytes())
        # for a pass over the streams of this call (TLSStreams): the device arrays as the assembler saw them
        self._last = dict(data=data, offsets=offsets, caplens=caplens, records=rec, layouts=lay, out=out, ids=ids,
                          stream=st)
        so = out["stream_of"][P:].cpu().tolist()
        result = dict(verdict=out["verdict"][P:].cpu().tolist(), stream_of=[ids[x] if x >= 0 else -1 for x in so],
                      streams=streams, data=out["data"], counts=counts)
        if self.timed:
            result["flushed"], result["closed"] = out["time_counts"].cpu().tolist()
            last_seen = out["conn_last_seen"][:G].cpu().tolist()
        # the state for the next call: per open connection its key's first packet
        # (CARRY_CONN), then its listed pages in list order (CARRY_PAGE | page)
        conn_seq = out["conn_seq"][:G].cpu().tolist()
        conn_stream = out["conn_stream"][:G].cpu().tolist()
        gfirst = groups["first"][:G].cpu().tolist()
        group_of = groups["group_of"].cpu().tolist()
        pend_pkt, pend_page = out["pend_pkt"][:NP].cpu().tolist(), out["pend_page"][:NP].cpu().tolist()
        order, ncode, nseq, ngid, norigin, nseen = [], [], [], [], [], []
        pages = {}
        for p, k in zip(pend_pkt, pend_page):
            pages.setdefault(group_of[p], []).append((p, k))
        for g in range(G):
            if conn_seq[g] == _lib.TCPASM_NO_CONN:
                continue
            order.append(gfirst[g])
            ncode.append(_lib.TCPASM_CARRY_CONN)
            nseq.append(conn_seq[g])
            ngid.append(ids[conn_stream[g]])
            norigin.append(origin(gfirst[g]))
            if self.timed:
                nseen.append(last_seen[g])
                nseen += [seen[p] for p, _ in pages.get(g, ())]
            for p, k in pages.get(g, ()):
                order.append(p)
                ncode.append(_lib.TCPASM_CARRY_PAGE | k)
                nseq.append(0)
                ngid.append(ids[conn_stream[g]])
                norigin.append(origin(p))
        if order:
            ot = torch.tensor(order, dtype=torch.int32, device=dev)
            self._carry = _pack_carry(data, offsets, caplens, ot, st) + (ncode, nseq, ngid, norigin)
            self._carry_seen = nseen if self.timed else None
        else:
            self._carry = self._carry_seen = None
        return result

    def close(self):
        self.grouper.close()
        self.assembler.close()


class Serializer(_Handle):
    """gpk_serialize_batch (include/gpk_serialize.h): gopacket.SerializeLayers for
    the packets of a decoded device batch, from their layouts and their (edited)
    gpk_fields records. Owns the handle and its scratch for up to max_packets
    output packets; device=None makes a host-only serializer (serialize_host)."""

    _create, _destroy = "gpk_serializer_create", "gpk_serializer_destroy"

    def __init__(self, max_packets=1, device=0):
        super().__init__(max_packets, -1 if device is None else int(device))

    def serialize(self, data, offsets, caplens, layouts, fields, order=None, fix_lengths=False,
                  compute_checksums=False, out=None, out_cap=None, group=0, stream=None):
        """Device tensors in: data uint8, offsets int64, caplens int32, layouts
        and fields the decode's (uint8 views of gpk_layout / gpk_fields), order
        int32 or None. Returns dict(out, offsets[m+1], caplens[m], status[m],
        err_args[2m], counts[4]) of device tensors; `out` may be given (uint8,
        its size is out_cap unless that is given too). A batch that does not fit
        has counts[3] set. With `out` or `out_cap` given, or without an order,
        nothing is synchronised here; with an order and neither of them the
        buffer is sized from the selected packets' lengths, which is one
        synchronising sum on the device."""
        import torch
        n = offsets.numel()
        m = n if order is None else order.numel()
        dev = offsets.device
        if out is None:
            if out_cap is None:
                # every packet keeps its bytes at most; headers grow by less than 64 + the Ethernet pad
                if order is None:
                    out_cap = int(data.numel()) + 128 * m
                else:  # a selection: the bytes it names (one synchronising sum)
                    sel = caplens.index_select(0, order.long().clamp(0, max(n - 1, 0)))
                    out_cap = int(sel.sum(dtype=torch.int64).item()) + 128 * m
            out = torch.empty(int(out_cap) + 16, dtype=torch.uint8, device=dev)
        elif out_cap is None:
            out_cap = out.numel()
        res = dict(out=out, offsets=torch.empty(m + 1, dtype=torch.int64, device=dev),
                   caplens=torch.empty(m, dtype=torch.int32, device=dev),
                   status=torch.empty(m, dtype=torch.int32, device=dev),
                   err_args=torch.zeros(2 * m, dtype=torch.int32, device=dev),
                   counts=torch.zeros(4, dtype=torch.int64, device=dev))
        b = _lib.Batch.of(data, offsets, caplens)
        o = _lib.SerializeOpts(int(bool(fix_lengths)), int(bool(compute_checksums)), int(group))
        sp = _lib.stream_ptr(stream)
        _lib.check(_lib.lib().gpk_serialize_batch(
            self.h, ctypes.byref(b), layouts.data_ptr(), fields.data_ptr(),
            order.data_ptr() if order is not None else None, m, ctypes.byref(o), out.data_ptr(), int(out_cap),
            res["offsets"].data_ptr(), res["caplens"].data_ptr(), res["status"].data_ptr(), res["err_args"].data_ptr(),
            res["counts"].data_ptr(), sp))
        return res

    def serialize_host(self, data, offsets, caplens, layouts, fields, order=None, fix_lengths=False,
                       compute_checksums=False, out_cap=None):
        """The same over numpy arrays (gpk_serialize_batch_host): data uint8,
        offsets uint64, caplens uint32, layouts _lib.LAYOUT_DTYPE, fields
        _lib.FIELDS_DTYPE, order uint32 or None."""
        import numpy as np
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        caplens = np.ascontiguousarray(caplens, np.uint32)
        layouts = np.ascontiguousarray(layouts, _lib.LAYOUT_DTYPE)
        fields = np.ascontiguousarray(fields, _lib.FIELDS_DTYPE)
        n = len(caplens)
        if order is not None:
            order = np.ascontiguousarray(order, np.uint32)
        m = n if order is None else len(order)
        if out_cap is None:
            idx = np.arange(n) if order is None else order[order < n]
            out_cap = int(caplens[idx].sum(dtype=np.uint64)) + 2300 * max(m, 1)
        res = dict(out=np.zeros(int(out_cap), np.uint8), offsets=np.zeros(m + 1, np.uint64),
                   caplens=np.zeros(m, np.uint32), status=np.zeros(m, np.int32), err_args=np.zeros(2 * m, np.uint32),
                   counts=np.zeros(4, np.uint64))
        b = _lib.Batch(data.ctypes.data, offsets.ctypes.data, caplens.ctypes.data, n, data.size)
        o = _lib.SerializeOpts(int(bool(fix_lengths)), int(bool(compute_checksums)), 0)
        _lib.check(_lib.lib().gpk_serialize_batch_host(
            self.h, ctypes.byref(b), layouts.ctypes.data, fields.ctypes.data,
            order.ctypes.data if order is not None else None, m, ctypes.byref(o), res["out"].ctypes.data, int(out_cap),
            res["offsets"].ctypes.data, res["caplens"].ctypes.data, res["status"].ctypes.data,
            res["err_args"].ctypes.data, res["counts"].ctypes.data))
        return res


def _per_packet(n):
    return n


def _per_entry(n):  # of the compact list: room for n, counts[0] of them written
    return n


class _PostPass(_Handle):
    """A pass over a decoded device batch that writes a compact list ordered by
    class (csrc/gpk_postpass.h). A subclass names its entry points, its _lib
    output struct, the flag that asks for the sums and OUTPUTS: (key, count for
    n packets, numpy dtype) of every array of that struct, in its order; the
    count of an array with one element per entry of the list is _per_entry."""

    _batch = _batch_host = _set_threshold = _Out = _FLAG = None
    OUTPUTS = ()

    def __init__(self, max_packets=1, device=0):
        if device is None:  # host-only: no handle
            self.h, self.max_packets = ctypes.c_void_p(), int(max_packets)
        else:
            super().__init__(max_packets, int(device))

    def set_sum_threshold(self, nbytes):
        """Lane group of the sums: 64 lanes from `nbytes` on, 16 below."""
        _lib.check(getattr(_lib.lib(), self._set_threshold)(self.h, int(nbytes)))

    def _device_outputs(self, n, dev):
        """The OUTPUTS arrays for n packets as device tensors: records as bytes, the rest as int32 / int64."""
        import numpy as np
        import torch
        out = {}
        for key, count, dt in self.OUTPUTS:
            dt = np.dtype(dt)
            out[key] = (torch.empty(count(n) * dt.itemsize, dtype=torch.uint8, device=dev) if dt.fields else
                        torch.empty(count(n), dtype=torch.int64 if dt.itemsize == 8 else torch.int32, device=dev))
        return out

    def _device(self, ctx, data, offsets, caplens, records, layouts, parser, kinds, sums, out, stream):
        if out is None:  # the call zeroes class_start and counts
            out = self._device_outputs(offsets.numel(), offsets.device)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        o = self._Out(*[out[key].data_ptr() for key, _, _ in self.OUTPUTS])
        entry = getattr(_lib.lib(), self._batch)
        _lib.check(entry(self.h, ctx.h, parser.h, ctypes.byref(b), ctypes.byref(r), int(kinds),
                         self._FLAG if sums else 0, ctypes.byref(o), _lib.stream_ptr(stream)))
        return out

    @classmethod
    def _host_arguments(cls, data, offsets, caplens, records, layouts, fill, extra=()):
        """(out, gpk_batch, gpk_results, the input arrays they point into): the
        OUTPUTS arrays for the batch, and `extra` (key, count, dtype) ones, all
        starting as `fill` bytes."""
        import numpy as np
        keep = (np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(offsets, np.uint64),
                np.ascontiguousarray(caplens, np.uint32), np.ascontiguousarray(records, _lib.RECORD_DTYPE),
                np.ascontiguousarray(layouts, _lib.LAYOUT_DTYPE))
        n = len(keep[2])
        out = {key: np.empty(count(n), dt) for key, count, dt in tuple(cls.OUTPUTS) + tuple(extra)}
        for a in out.values():
            a.view(np.uint8)[:] = fill
        b = _lib.Batch(keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, n, keep[0].size)
        r = _lib.Results(keep[3].ctypes.data, None, None, keep[4].ctypes.data)
        return out, b, r, keep

    @classmethod
    def _host(cls, data, offsets, caplens, records, layouts, parser, kinds, sums, fill):
        out, b, r, _keep = cls._host_arguments(data, offsets, caplens, records, layouts, fill)
        o = cls._Out(*[out[key].ctypes.data for key, _, _ in cls.OUTPUTS])
        _lib.check(getattr(_lib.lib(), cls._batch_host)(parser.h, ctypes.byref(b), ctypes.byref(r), int(kinds),
                                                        cls._FLAG if sums else 0, ctypes.byref(o)))
        return out

    @classmethod
    def to_host(cls, out):
        """A device result as numpy arrays of the OUTPUTS dtypes, cut to what
        the call wrote: the per-entry arrays to counts[0] entries, the others
        whole. Synchronizes."""
        import numpy as np
        m = int(out["counts"][0].item())
        host = {}
        for key, count, dt in cls.OUTPUTS:
            dt = np.dtype(dt)
            t = out[key][:m * (dt.itemsize if dt.fields else 1)] if count is _per_entry else out[key]
            host[key] = t.cpu().numpy().view(dt)
        return host


class _ArenaPass(_PostPass):
    """A _PostPass whose result has a variable length (csrc/gpk_arena.h): the
    entries name ranges of arenas of the caller's capacities. A subclass adds
    ARENAS: (key, numpy dtype, the first of the two counts words that hold its
    need) of every arena, in the order of the output struct, which ends with
    their pointers and then their capacities. `batch` is (data, offsets,
    caplens, records, layouts, parser), `caps` a capacity per arena, `kinds`
    None where the entry points take none."""

    ARENAS = ()

    @classmethod
    def _needs(cls, counts):
        c = [int(x) & 0xffffffff for x in counts]
        return tuple(c[w] | c[w + 1] << 32 for _, _, w in cls.ARENAS)

    @classmethod
    def needed(cls, counts):
        """What the batch needs of each arena, from counts (uint32): a tuple in
        the order of the capacities, or the one number where there is one."""
        needs = cls._needs(counts)
        return needs if len(needs) > 1 else needs[0]

    @classmethod
    def _out_struct(cls, out, caps, ptr):
        return cls._Out(*[ptr(out[key]) for key, _, _ in cls.OUTPUTS],
                        *[ptr(out[key]) if cap else None for (key, _, _), cap in zip(cls.ARENAS, caps)], *caps)

    def _decode(self, ctx, batch, caps, kinds, out, stream):
        import numpy as np
        import torch
        data, offsets, caplens, records, layouts, parser = batch
        caps = [int(cap) for cap in caps]
        if out is None:
            dev = offsets.device
            out = self._device_outputs(offsets.numel(), dev)
            for (key, dt, _), cap in zip(self.ARENAS, caps):
                out[key] = torch.empty(cap * np.dtype(dt).itemsize, dtype=torch.uint8, device=dev)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        o = self._out_struct(out, caps, lambda t: t.data_ptr())
        _lib.check(getattr(_lib.lib(), self._batch)(
            self.h, ctx.h, parser.h, ctypes.byref(b), ctypes.byref(r), *(() if kinds is None else (int(kinds),)),
            ctypes.byref(o), _lib.stream_ptr(stream)))
        return out

    def _decode_all(self, ctx, batch, caps, kinds, stream):
        out = self._decode(ctx, batch, caps, kinds, None, stream)
        counts = out["counts"].cpu().numpy().view("u4")
        if int(counts[3]):
            out = self._decode(ctx, batch, self._needs(counts), kinds, None, stream)
        return out

    @classmethod
    def _decode_host(cls, batch, caps, kinds, fill=0):
        caps = [int(cap) for cap in caps]
        out, b, r, _keep = cls._host_arguments(
            *batch[:5], fill, [(key, lambda n, cap=cap: cap, dt) for (key, dt, _), cap in zip(cls.ARENAS, caps)])
        o = cls._out_struct(out, caps, lambda a: a.ctypes.data)
        _lib.check(getattr(_lib.lib(), cls._batch_host)(
            batch[5].h, ctypes.byref(b), ctypes.byref(r), *(() if kinds is None else (int(kinds),)), ctypes.byref(o)))
        return out

    @classmethod
    def _decode_host_all(cls, batch, caps, kinds):
        out = cls._decode_host(batch, caps, kinds)
        if int(out["counts"][3]):
            out = cls._decode_host(batch, cls._needs(out["counts"]), kinds)
        return out

    @classmethod
    def to_host(cls, out):
        """_PostPass.to_host, and each arena cut to what the batch needs."""
        import numpy as np
        host = super().to_host(out)
        for (key, dt, _), need in zip(cls.ARENAS, cls._needs(host["counts"])):
            host[key] = out[key][:need * np.dtype(dt).itemsize].cpu().numpy().view(dt)
        return host


class Detunneler(_PostPass):
    """gpk_tunnel_batch (include/gpk_tunnel.h): one tunnel level peeled off a
    decoded device batch. Owns the workspace of the scans for up to max_packets
    packets; device=None makes a host-only one (peel_host)."""

    _create, _destroy = "gpk_tunneler_create", "gpk_tunneler_destroy"
    _batch, _batch_host, _set_threshold = "gpk_tunnel_batch", "gpk_tunnel_batch_host", "gpk_tunneler_set_sum_threshold"
    _Out, _FLAG = _lib.Tunnels, _lib.TUN_GRE_CSUM
    OUTPUTS = (("verdict", _per_packet, "i4"), ("class_start", lambda n: 7, "u4"), ("index", _per_entry, "u4"),
               ("in_offsets", _per_entry, "u8"), ("in_caplens", _per_entry, "u4"),
               ("tunnels", _per_entry, _lib.TUNNEL_DTYPE), ("counts", lambda n: 8, "u4"))
    KEYS = tuple(k for k, _, _ in OUTPUTS)

    def peel(self, ctx, data, offsets, caplens, records, layouts, parser, kinds=_lib.TUN_ALL, gre_checksum=True,
             out=None, stream=None):
        """Device tensors in: the batch, and the records and layouts of
        ctx.decode_device(parser, ...) for it. Returns dict(verdict[n],
        class_start[7], index[n], in_offsets[n], in_caplens[n], tunnels[72 n]
        (uint8, _lib.TUNNEL_DTYPE), counts[8]) of device tensors (or fills
        `out`); entries at and past counts[0] are not written. Class c's inner
        batch is (data, in_offsets[class_start[c]:class_start[c+1]],
        in_caplens[...]) for a parser whose first layer is the class's type."""
        return self._device(ctx, data, offsets, caplens, records, layouts, parser, kinds, gre_checksum, out, stream)

    @classmethod
    def peel_host(cls, data, offsets, caplens, records, layouts, parser, kinds=_lib.TUN_ALL, gre_checksum=True, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_tunnel_batch_host); `fill` is the byte the outputs start with."""
        return cls._host(data, offsets, caplens, records, layouts, parser, kinds, gre_checksum, fill)


class ControlDecoder(_PostPass):
    """gpk_control_batch (include/gpk_control.h): the ICMPv4, ICMPv6,
    ICMPv6Echo and ARP layers at the end of a decoded device batch. Owns the
    workspace of the scans for up to max_packets packets; device=None makes a
    host-only one (decode_host)."""

    _create, _destroy = "gpk_controller_create", "gpk_controller_destroy"
    _batch, _batch_host = "gpk_control_batch", "gpk_control_batch_host"
    _set_threshold = "gpk_controller_set_sum_threshold"
    _Out, _FLAG = _lib.Controls, _lib.CTL_CSUM
    OUTPUTS = (("verdict", _per_packet, "i4"), ("class_start", lambda n: 5, "u4"), ("index", _per_entry, "u4"),
               ("records", _per_entry, _lib.CONTROL_DTYPE), ("counts", lambda n: 8, "u4"))
    KEYS = tuple(k for k, _, _ in OUTPUTS)

    def decode(self, ctx, data, offsets, caplens, records, layouts, parser, kinds=_lib.CTL_ALL, checksum=True,
               out=None, stream=None):
        """Device tensors in: the batch (data 16-byte aligned and readable to
        the next 16-byte boundary past its last packet), and the records and
        layouts of ctx.decode_device(parser, ...) for it. Returns
        dict(verdict[n], class_start[5], index[n], records[64 n] (uint8,
        _lib.CONTROL_DTYPE), counts[8]) of device tensors (or fills `out`);
        entries at and past counts[0] are not written."""
        return self._device(ctx, data, offsets, caplens, records, layouts, parser, kinds, checksum, out, stream)

    @classmethod
    def decode_host(cls, data, offsets, caplens, records, layouts, parser, kinds=_lib.CTL_ALL, checksum=True, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_control_batch_host); `fill` is the byte the outputs start with."""
        return cls._host(data, offsets, caplens, records, layouts, parser, kinds, checksum, fill)


class DNSDecoder(_ArenaPass):
    """gpk_dns_batch (include/gpk_dns.h): the DNS messages at the end of a
    decoded device batch. Owns the workspace of the scans for up to
    max_packets packets; device=None makes a host-only one (decode_host).

    The result is variable-length: records[m] (DNS_DTYPE) name ranges of
    rrs[rr_cap] (DNS_RR_DTYPE) and of the byte arena names[name_cap]. A message
    whose range does not fit either capacity is not written (DNS_ST_DROPPED);
    counts tells what the batch needs (needed()), and decode_all /
    decode_host_all size first and decode once more with exactly that."""

    _create, _destroy = "gpk_dns_decoder_create", "gpk_dns_decoder_destroy"
    _batch, _batch_host, _Out = "gpk_dns_batch", "gpk_dns_batch_host", _lib.Dnss
    OUTPUTS = (("verdict", _per_packet, "i4"), ("class_start", lambda n: 3, "u4"), ("index", _per_entry, "u4"),
               ("records", _per_entry, _lib.DNS_DTYPE), ("counts", lambda n: 8, "u4"))
    ARENAS = (("rrs", _lib.DNS_RR_DTYPE, 4), ("names", "u1", 6))
    KEYS = tuple(k for k, _, _ in OUTPUTS + ARENAS)

    def decode(self, ctx, data, offsets, caplens, records, layouts, parser, rr_cap, name_cap, out=None, stream=None):
        """Device tensors in: the batch (data 16-byte aligned), and the records
        and layouts of ctx.decode_device(parser, ...) for it. Returns
        dict(verdict[n], class_start[3], index[n], records[64 n] (uint8,
        _lib.DNS_DTYPE), counts[8], rrs[96 rr_cap] (uint8, _lib.DNS_RR_DTYPE),
        names[name_cap] (uint8)) of device tensors (or fills `out`); entries at
        and past counts[0] are not written, nor is anything past a capacity."""
        return self._decode(ctx, (data, offsets, caplens, records, layouts, parser), (rr_cap, name_cap), None, out, stream)

    def decode_all(self, ctx, data, offsets, caplens, records, layouts, parser, rr_cap=0, name_cap=0, stream=None):
        """decode with capacities that hold every message: a first call with
        rr_cap / name_cap, and, when counts reports an overflow, a second one
        with exactly the sizes it needs. With the default capacities of 0 the
        first call only sizes: no memory is set aside on a guess, at the price
        of a second pass whenever the batch holds a message that decodes.
        Synchronizes on the counts."""
        return self._decode_all(ctx, (data, offsets, caplens, records, layouts, parser), (rr_cap, name_cap), None, stream)

    @classmethod
    def decode_host(cls, data, offsets, caplens, records, layouts, parser, rr_cap, name_cap, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_dns_batch_host); `fill` is the byte the outputs start with."""
        return cls._decode_host((data, offsets, caplens, records, layouts, parser), (rr_cap, name_cap), None, fill)

    @classmethod
    def decode_host_all(cls, data, offsets, caplens, records, layouts, parser, rr_cap=0, name_cap=0):
        """decode_host with the retry of decode_all."""
        return cls._decode_host_all((data, offsets, caplens, records, layouts, parser), (rr_cap, name_cap), None)


class NDPDecoder(_ArenaPass):
    """gpk_ndp_batch (include/gpk_ndp.h): the NDP and MLD messages behind
    ICMPv6 at the end of a decoded device batch. Owns the workspace of the
    scans for up to max_packets packets; device=None makes a host-only one
    (decode_host).

    The result is variable-length: records[m] (NDP_DTYPE) name ranges of
    entries[entry_cap] (NDP_ENTRY_DTYPE), one per option or multicast address
    record. A message whose range does not fit is not written
    (NDP_ST_DROPPED); counts tells what the batch needs (needed()), and
    decode_all / decode_host_all size first and decode once more with exactly
    that."""

    _create, _destroy = "gpk_ndp_decoder_create", "gpk_ndp_decoder_destroy"
    _batch, _batch_host, _Out = "gpk_ndp_batch", "gpk_ndp_batch_host", _lib.Ndps
    OUTPUTS = (("verdict", _per_packet, "i4"), ("class_start", lambda n: 3, "u4"), ("index", _per_entry, "u4"),
               ("records", _per_entry, _lib.NDP_DTYPE), ("counts", lambda n: 8, "u4"))
    ARENAS = (("entries", _lib.NDP_ENTRY_DTYPE, 4),)
    KEYS = tuple(k for k, _, _ in OUTPUTS + ARENAS)

    def decode(self, ctx, data, offsets, caplens, records, layouts, parser, entry_cap, kinds=_lib.NDP_ALL, out=None,
               stream=None):
        """Device tensors in: the batch (data 16-byte aligned), and the records
        and layouts of ctx.decode_device(parser, ...) for it. kinds: NDP_* mask
        of the layers the caller's parser holds. Returns dict(verdict[n],
        class_start[3], index[n], records[64 n] (uint8, _lib.NDP_DTYPE),
        counts[8], entries[16 entry_cap] (uint8, _lib.NDP_ENTRY_DTYPE)) of
        device tensors (or fills `out`); entries at and past counts[0] are not
        written, nor is anything past the capacity."""
        return self._decode(ctx, (data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds, out, stream)

    def decode_all(self, ctx, data, offsets, caplens, records, layouts, parser, entry_cap=0, kinds=_lib.NDP_ALL,
                   stream=None):
        """decode with a capacity that holds every message: a first call with
        entry_cap, and, when counts reports an overflow, a second one with
        exactly the size it needs. With the default capacity of 0 the first
        call only sizes. Synchronizes on the counts."""
        return self._decode_all(ctx, (data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds, stream)

    @classmethod
    def decode_host(cls, data, offsets, caplens, records, layouts, parser, entry_cap, kinds=_lib.NDP_ALL, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_ndp_batch_host); `fill` is the byte the outputs start with."""
        return cls._decode_host((data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds, fill)

    @classmethod
    def decode_host_all(cls, data, offsets, caplens, records, layouts, parser, entry_cap=0, kinds=_lib.NDP_ALL):
        """decode_host with the retry of decode_all."""
        return cls._decode_host_all((data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds)


class ServiceDecoder(_ArenaPass):
    """gpk_svc_batch (include/gpk_svc.h): the DHCPv4, DHCPv6 and NTP
    messages at the end of a decoded device batch. Owns the workspace of the
    scans for up to max_packets packets; device=None makes a host-only one
    (decode_host).

    The result is variable-length: records[m] (SVC_DTYPE) name ranges of
    entries[entry_cap] (SVC_ENTRY_DTYPE), one per DHCP option. A message
    whose range does not fit is not written (SVC_ST_DROPPED); counts tells
    what the batch needs (needed()), and
    decode_all / decode_host_all size first and decode once more with exactly
    that."""

    _create, _destroy = "gpk_svc_decoder_create", "gpk_svc_decoder_destroy"
    _batch, _batch_host, _Out = "gpk_svc_batch", "gpk_svc_batch_host", _lib.Svcs
    OUTPUTS = (("verdict", _per_packet, "i4"), ("class_start", lambda n: 3, "u4"), ("index", _per_entry, "u4"),
               ("records", _per_entry, _lib.SVC_DTYPE), ("counts", lambda n: 8, "u4"))
    ARENAS = (("entries", _lib.SVC_ENTRY_DTYPE, 4),)
    KEYS = tuple(k for k, _, _ in OUTPUTS + ARENAS)

    def decode(self, ctx, data, offsets, caplens, records, layouts, parser, entry_cap, kinds=_lib.SVC_ALL, out=None,
               stream=None):
        """Device tensors in: the batch (data 16-byte aligned), and the records
        and layouts of ctx.decode_device(parser, ...) for it. kinds: SVC_* mask
        of the layers the caller's parser holds. Returns dict(verdict[n],
        class_start[3], index[n], records[64 n] (uint8, _lib.SVC_DTYPE),
        counts[8], entries[8 entry_cap] (uint8, _lib.SVC_ENTRY_DTYPE)) of
        device tensors (or fills `out`); entries at and past counts[0] are not
        written, nor is anything past the capacity."""
        return self._decode(ctx, (data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds, out, stream)

    def decode_all(self, ctx, data, offsets, caplens, records, layouts, parser, entry_cap=0, kinds=_lib.SVC_ALL,
                   stream=None):
        """decode with a capacity that holds every message: a first call with
        entry_cap, and, when counts reports an overflow, a second one with
        exactly the size it needs. With the default capacity of 0 the first
        call only sizes. Synchronizes on the counts."""
        return self._decode_all(ctx, (data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds, stream)

    @classmethod
    def decode_host(cls, data, offsets, caplens, records, layouts, parser, entry_cap, kinds=_lib.SVC_ALL, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_svc_batch_host); `fill` is the byte the outputs start with."""
        return cls._decode_host((data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds, fill)

    @classmethod
    def decode_host_all(cls, data, offsets, caplens, records, layouts, parser, entry_cap=0, kinds=_lib.SVC_ALL):
        """decode_host with the retry of decode_all."""
        return cls._decode_host_all((data, offsets, caplens, records, layouts, parser), (entry_cap,), kinds)


class TLSDecoder(_ArenaPass):
    """gpk_tls_batch (include/gpk_tls.h): the TLS messages at the end of a
    decoded device batch. Owns the workspace of the scans for up to
    max_packets packets; device=None makes a host-only one (decode_host).

    The result is variable-length: records[m] (TLS_DTYPE) name ranges of
    recs[rec_cap] (TLS_REC_DTYPE, one per TLS record), of hellos[hello_cap]
    (TLS_HELLO_DTYPE, one per decoded ClientHello) and of the byte arena
    snis[sni_cap] (the server names). A message whose range does not fit every
    capacity is not written (TLS_ST_DROPPED); counts tells what the batch
    needs (needed()), and decode_all / decode_host_all size first and decode
    once more with exactly that."""

    _create, _destroy = "gpk_tls_decoder_create", "gpk_tls_decoder_destroy"
    _batch, _batch_host, _Out = "gpk_tls_batch", "gpk_tls_batch_host", _lib.Tlss
    OUTPUTS = (("verdict", _per_packet, "i4"), ("class_start", lambda n: 3, "u4"), ("index", _per_entry, "u4"),
               ("records", _per_entry, _lib.TLS_DTYPE), ("counts", lambda n: 12, "u4"))
    ARENAS = (("recs", _lib.TLS_REC_DTYPE, 4), ("hellos", _lib.TLS_HELLO_DTYPE, 6), ("snis", "u1", 8))
    KEYS = tuple(k for k, _, _ in OUTPUTS + ARENAS)

    def decode(self, ctx, data, offsets, caplens, records, layouts, parser, rec_cap, hello_cap, sni_cap, out=None,
               stream=None):
        """Device tensors in: the batch (data 16-byte aligned), and the records
        and layouts of ctx.decode_device(parser, ...) for it. Returns
        dict(verdict[n], class_start[3], index[n], records[80 n] (uint8,
        _lib.TLS_DTYPE), counts[12], recs[16 rec_cap] (uint8,
        _lib.TLS_REC_DTYPE), hellos[64 hello_cap] (uint8,
        _lib.TLS_HELLO_DTYPE), snis[sni_cap] (uint8)) of device tensors (or
        fills `out`); entries at and past counts[0] are not written, nor is
        anything past a capacity."""
        return self._decode(ctx, (data, offsets, caplens, records, layouts, parser), (rec_cap, hello_cap, sni_cap), None,
                            out, stream)

    def decode_all(self, ctx, data, offsets, caplens, records, layouts, parser, rec_cap=0, hello_cap=0, sni_cap=0,
                   stream=None):
        """decode with capacities that hold every message: a first call with
        the capacities given, and, when counts reports an overflow, a second
        one with exactly the sizes it needs. With the default capacities of 0
        the first call only sizes. Synchronizes on the counts."""
        return self._decode_all(ctx, (data, offsets, caplens, records, layouts, parser), (rec_cap, hello_cap, sni_cap),
                                None, stream)

    @classmethod
    def decode_host(cls, data, offsets, caplens, records, layouts, parser, rec_cap, hello_cap, sni_cap, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_tls_batch_host); `fill` is the byte the outputs start with."""
        return cls._decode_host((data, offsets, caplens, records, layouts, parser), (rec_cap, hello_cap, sni_cap), None,
                                fill)

    @classmethod
    def decode_host_all(cls, data, offsets, caplens, records, layouts, parser, rec_cap=0, hello_cap=0, sni_cap=0):
        """decode_host with the retry of decode_all."""
        return cls._decode_host_all((data, offsets, caplens, records, layouts, parser), (rec_cap, hello_cap, sni_cap),
                                    None)


class TLSStreamDecoder(_Handle):
    """gpk_tls_streams (include/gpk_tls_streams.h): the TLS records of the
    streams of one Assembler.assemble call. Owns the workspace of the scans for
    calls of up to max_streams packets; device=None makes a host-only one
    (decode_host).

    The result is variable-length: streams[S] (TLS_STREAM_DTYPE) name ranges
    of recs[rec_cap] (TLS_STREAM_REC_DTYPE, one per TLS record), of
    hellos[hello_cap] (TLS_HELLO_DTYPE; packet holds the stream's index), of
    the byte arena snis[sni_cap] and of the tail arena tails[tail_cap]. A
    stream whose range does not fit every capacity is not written
    (TLSS_ST_DROPPED); counts tells what the call needs (needed()), and
    decode_all / decode_host_all size first and decode once more with exactly
    that. `carry` is (state, tail_off, tail_len, tails) of the call's first
    len(state) streams: uint32 / int32 states, int64 offsets and int32 lengths
    into the uint8 arena `tails` (the `tails` output of the call before, which
    must not be this call's output arena)."""

    _create, _destroy = "gpk_tls_stream_decoder_create", "gpk_tls_stream_decoder_destroy"
    KEYS = ("streams", "recs", "hellos", "snis", "tails", "counts")
    ASM_KEYS = ("verdict", "stream_of", "chunks", "stream_group", "stream_first", "stream_closed", "stream_chunk0",
                "stream_data0", "conn_seq", "conn_stream", "pend_pkt", "pend_page", "counts", "data")

    def __init__(self, max_streams=1, device=0):
        if device is None:  # host-only: no handle
            self.h, self.max_packets = ctypes.c_void_p(), int(max_streams)
        else:
            super().__init__(max_streams, int(device))

    @staticmethod
    def needed(counts):
        """(record entries, hello entries, server name bytes, tail bytes) the call needs, from counts[12]."""
        return tuple(int(x) for x in counts[6:10])

    @staticmethod
    def _structs(ptr, numel, asm, carry, caps, out, frame_unstarted):
        a = _lib.TcpStreams(*[ptr(asm[k]) if asm.get(k) is not None else None for k in TLSStreamDecoder.ASM_KEYS],
                            int(asm.get("chunk_cap", numel(asm["chunks"]) // _lib.TCP_CHUNK_DTYPE.itemsize)),
                            int(asm.get("data_cap", numel(asm["data"]))))
        flags = _lib.TLSS_FRAME_UNSTARTED if frame_unstarted else 0
        if carry is None:
            i = _lib.TlsStreamIn(None, None, None, None, 0, 0, flags, 0)
        else:
            state, off, ln, tails = carry
            nt = 0 if tails is None else numel(tails)
            i = _lib.TlsStreamIn(ptr(state), ptr(off), ptr(ln), ptr(tails) if nt else None, numel(state), nt, flags, 0)
        o = _lib.TlsStreamOut(ptr(out["streams"]), *[ptr(out[k]) if c else None for k, c in
                                                     zip(("recs", "hellos", "snis", "tails"), caps)],
                              ptr(out["counts"]), *caps)
        return a, i, o

    def decode(self, ctx, parser, data, offsets, caplens, records, layouts, asm, rec_cap, hello_cap, sni_cap, tail_cap,
               carry=None, frame_unstarted=False, out=None, stream=None):
        """Device tensors in: the batch the assembler was given, its records
        and layouts, and `asm`, the dict Assembler.assemble returned for it.
        Returns dict(streams[64 n] (uint8, _lib.TLS_STREAM_DTYPE), recs[32
        rec_cap] (uint8, _lib.TLS_STREAM_REC_DTYPE), hellos[64 hello_cap],
        snis[sni_cap], tails[tail_cap], counts[12] (int64)) of device tensors
        (or fills `out`); stream entries at and past counts[0] are not written,
        nor is anything past a capacity. Asynchronous on `stream`."""
        import torch
        caps = (int(rec_cap), int(hello_cap), int(sni_cap), int(tail_cap))
        n, dev = offsets.numel(), offsets.device
        if out is None:
            u8 = torch.uint8
            out = dict(streams=torch.empty(max(n, 1) * 64, dtype=u8, device=dev),
                       recs=torch.empty(caps[0] * 32, dtype=u8, device=dev),
                       hellos=torch.empty(caps[1] * 64, dtype=u8, device=dev),
                       snis=torch.empty(caps[2], dtype=u8, device=dev), tails=torch.empty(caps[3], dtype=u8, device=dev),
                       counts=torch.zeros(12, dtype=torch.int64, device=dev))
        a, i, o = self._structs(lambda t: t.data_ptr(), lambda t: t.numel(), asm, carry, caps, out, frame_unstarted)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        _lib.check(_lib.lib().gpk_tls_streams(self.h, ctx.h, parser.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(a),
                                              ctypes.byref(i), ctypes.byref(o), _lib.stream_ptr(stream)))
        return out

    def decode_all(self, ctx, parser, data, offsets, caplens, records, layouts, asm, rec_cap=0, hello_cap=0, sni_cap=0,
                   tail_cap=0, carry=None, frame_unstarted=False, stream=None):
        """decode with capacities that hold every stream: a first call with the
        capacities given, and, when counts reports an overflow, a second one
        with exactly the sizes it needs. With the default capacities of 0 the
        first call only sizes. Synchronizes on the counts."""
        out = self.decode(ctx, parser, data, offsets, caplens, records, layouts, asm, rec_cap, hello_cap, sni_cap,
                          tail_cap, carry, frame_unstarted, stream=stream)
        counts = out["counts"].cpu().tolist()
        if counts[5]:
            out = self.decode(ctx, parser, data, offsets, caplens, records, layouts, asm, *self.needed(counts),
                              carry=carry, frame_unstarted=frame_unstarted, stream=stream)
        return out

    @classmethod
    def decode_host(cls, parser, data, offsets, caplens, records, layouts, asm, rec_cap, hello_cap, sni_cap, tail_cap,
                    carry=None, frame_unstarted=False, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_tls_streams_host); asm holds the assembler's outputs as numpy
        arrays (chunks as _lib.TCP_CHUNK_DTYPE, stream_first, stream_closed,
        stream_data0, counts, data at least); `fill` is the byte the outputs
        start with."""
        import numpy as np
        caps = (int(rec_cap), int(hello_cap), int(sni_cap), int(tail_cap))
        keep = (np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(offsets, np.uint64),
                np.ascontiguousarray(caplens, np.uint32), np.ascontiguousarray(records, _lib.RECORD_DTYPE),
                np.ascontiguousarray(layouts, _lib.LAYOUT_DTYPE))
        n = len(keep[2])
        asm = dict(asm)
        for k, dt in (("chunks", _lib.TCP_CHUNK_DTYPE), ("stream_first", np.uint32), ("stream_closed", np.uint32),
                      ("stream_data0", np.uint64), ("counts", np.uint64), ("data", np.uint8)):
            asm[k] = np.ascontiguousarray(asm[k], dt)
        asm.setdefault("chunk_cap", len(asm["chunks"]))
        asm.setdefault("data_cap", len(asm["data"]))
        if carry is not None:
            carry = (np.ascontiguousarray(carry[0], np.uint32), np.ascontiguousarray(carry[1], np.uint64),
                     np.ascontiguousarray(carry[2], np.uint32),
                     None if carry[3] is None else np.ascontiguousarray(carry[3], np.uint8))
        out = dict(streams=np.empty(max(n, 1), _lib.TLS_STREAM_DTYPE), recs=np.empty(caps[0], _lib.TLS_STREAM_REC_DTYPE),
                   hellos=np.empty(caps[1], _lib.TLS_HELLO_DTYPE), snis=np.empty(caps[2], np.uint8),
                   tails=np.empty(caps[3], np.uint8), counts=np.empty(12, np.uint64))
        for v in out.values():
            v.view(np.uint8)[:] = fill
        a, i, o = cls._structs(lambda t: t.ctypes.data, lambda t: t.size, asm, carry, caps, out, frame_unstarted)
        b = _lib.Batch(keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, n, keep[0].size)
        r = _lib.Results(keep[3].ctypes.data, None, None, keep[4].ctypes.data)
        _lib.check(_lib.lib().gpk_tls_streams_host(parser.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(a),
                                                   ctypes.byref(i), ctypes.byref(o)))
        return out

    @classmethod
    def decode_host_all(cls, parser, data, offsets, caplens, records, layouts, asm, rec_cap=0, hello_cap=0, sni_cap=0,
                        tail_cap=0, carry=None, frame_unstarted=False):
        """decode_host with the retry of decode_all."""
        out = cls.decode_host(parser, data, offsets, caplens, records, layouts, asm, rec_cap, hello_cap, sni_cap,
                              tail_cap, carry, frame_unstarted)
        if int(out["counts"][5]):
            out = cls.decode_host(parser, data, offsets, caplens, records, layouts, asm, *cls.needed(out["counts"]),
                                  carry=carry, frame_unstarted=frame_unstarted)
        return out


class TLSStreamResult:
    """What TLSStreams returns for one call. streams: [dict(id (global),
    state (TLSS_*), status, tail_in, recs (TLS_STREAM_REC_DTYPE), hellos
    (TLS_HELLO_DTYPE), names ([bytes or None] per hello), closed, and key with
    keys=True on a new stream)]; offsets of recs and hellos are relative to
    the stream's logical buffer of this call (tail_in carried bytes, then the
    new ones). counts: gpk_tls_stream_out.counts. Only these tables and the
    names come to the host, no stream byte."""

    def __init__(self, streams, counts, assembled):
        self.streams, self.counts, self.assembled = streams, counts, assembled

    def snis(self):
        """[(global stream id, server name)] in stream order."""
        return [(s["id"], nm) for s in self.streams for nm in s["names"] if nm is not None]


class _StreamPass:
    """What TLSStreams and DNSStreams share: a TCPAssembler in front and a
    stream decoder behind it, over a stream of device batches. The state and
    the unfinished tail of every open stream are kept per global stream id; the
    tails stay on the device. Every open connection is a stream of every call
    (it goes in as a carried entry), so the tail arena of one call is the input
    arena of the next. A closed stream's state is dropped. A subclass names its
    decoder (_new_decoder), the state of a new stream (_NEW) and decodes one
    call (_decode)."""
    _NEW = 0

    def __init__(self, ctx, parser, max_packets, max_pages=0, timed=False, frame_unstarted=False, device=0, keys=False):
        self.ctx, self.parser = ctx, parser
        self.asm = TCPAssembler(ctx, parser, max_packets, max_pages=max_pages, device=device, keys=keys, timed=timed)
        self.frame_unstarted = bool(frame_unstarted)
        self.device = device
        self.decoder = self._new_decoder()
        self._state = {}    # global id -> (state, tail_off, tail_len) into _tails
        self._tails = None

    def feed(self, data, offsets, caplens, timestamps=None):
        """One batch (as TCPAssembler.assemble). Returns the pass's result object."""
        return self._decode(self.asm.assemble(data, offsets, caplens, timestamps))

    def flush_all(self):
        return self._decode(self.asm.flush_all())

    def flush_older_than(self, t):
        return self._decode(self.asm.flush_older_than(t))

    def _carry_in(self):
        """(the assembler's last call, carry) for the decoder: what the call's
        streams had after the call before, in stream order."""
        import numpy as np
        import torch
        last = self.asm._last
        ids = last["ids"]
        if last["offsets"].numel() > self.decoder.max_packets:  # the assembler grew its workspaces
            self.decoder.close()
            self.decoder = self._new_decoder()
        dev = last["offsets"].device
        st = np.zeros((3, len(ids)), np.int64)
        for j, g in enumerate(ids):
            st[:, j] = self._state.get(g, (self._NEW, 0, 0))
        carry = (torch.tensor(st[0], dtype=torch.int32, device=dev), torch.tensor(st[1], dtype=torch.int64, device=dev),
                 torch.tensor(st[2], dtype=torch.int32, device=dev), self._tails)
        return last, carry

    def _carry_out(self, ids, ent, assembled, tails):
        """Keep what the call left: ent[j] is stream j's entry (state, tail_off, tail_len)."""
        self._tails = tails
        for g, e, a in zip(ids, ent, assembled):
            if a["closed"] is not None:
                self._state.pop(g, None)
            else:
                self._state[g] = (int(e["state"]), int(e["tail_off"]), int(e["tail_len"]))

    def close(self):
        self.asm.close()
        self.decoder.close()


class TLSStreams(_StreamPass):
    """TLS over reassembled streams: a TCPAssembler and a TLSStreamDecoder
    behind it, over a stream of device batches. The state and the unfinished
    tail of every open stream are kept per global stream id; the tails stay on
    the device. Every open connection is a stream of every call (it goes in as
    a carried entry), so the tail arena of one call is the input arena of the
    next. A closed stream's state is dropped."""
    _NEW = _lib.TLSS_NEW

    def _new_decoder(self):
        return TLSStreamDecoder(self.asm.max_packets, self.device)

    def _decode(self, res):
        if self.asm._last is None or not res["streams"]:
            return TLSStreamResult([], [0] * 12, res)
        last, carry = self._carry_in()
        ids = last["ids"]
        S = len(ids)
        out = self.decoder.decode_all(self.ctx, self.parser, last["data"], last["offsets"], last["caplens"],
                                      last["records"], last["layouts"], last["out"], carry=carry,
                                      frame_unstarted=self.frame_unstarted, stream=last["stream"])
        self._last_call = dict(carry=carry, out=out)  # what went in beside asm._last, and what came out
        counts = out["counts"].cpu().tolist()
        ent = out["streams"].cpu().numpy().view(_lib.TLS_STREAM_DTYPE)[:S]
        recs = out["recs"].cpu().numpy().view(_lib.TLS_STREAM_REC_DTYPE)
        hellos = out["hellos"].cpu().numpy().view(_lib.TLS_HELLO_DTYPE)
        snis = out["snis"].cpu().numpy()
        streams = []
        for j, (g, e, a) in enumerate(zip(ids, ent, res["streams"])):
            r0, h0 = int(e["rec0"]), int(e["hello0"])
            hs = hellos[h0:h0 + int(e["nhello"])]
            names = [bytes(snis[int(h["sni_pos"]):int(h["sni_pos"]) + int(h["sni_len"])]) if int(h["has_sni"]) else None
                     for h in hs]
            d = dict(id=g, state=int(e["state"]), status=int(e["status"]), tail_in=int(e["tail_in"]),
                     recs=recs[r0:r0 + int(e["nrec"])], hellos=hs, names=names, closed=a["closed"])
            if "key" in a:
                d["key"] = a["key"]
            streams.append(d)
        self._carry_out(ids, ent, res["streams"], out["tails"])
        return TLSStreamResult(streams, counts, res)


class DNSStreamDecoder(_Handle):
    """gpk_dns_streams (include/gpk_dns_streams.h): the DNS messages of the
    streams of one Assembler.assemble call. Owns the workspace of the scans for
    calls of up to max_streams packets and msg_cap <= max_msgs message entries;
    device=None makes a host-only one (decode_host).

    The result is variable-length on two levels: streams[S] (DNS_STREAM_DTYPE)
    name ranges of msgs[msg_cap] (DNS_STREAM_MSG_DTYPE, one per message) and of
    the tail arena tails[tail_cap]; a stream whose range does not fit is not
    written (DNSS_ST_DROPPED). A message names ranges of rrs[rr_cap]
    (DNS_RR_DTYPE) and of the byte arena names[name_cap]; a message whose range
    does not fit is not written (DNSS_MSG_DROPPED). counts tells what the call
    needs (needed()); the rr and name needs are those of the placed messages,
    so decode_all / decode_host_all size the streams first, then the messages,
    and decode once more. `carry` is as for TLSStreamDecoder."""

    _create, _destroy = "gpk_dns_stream_decoder_create", "gpk_dns_stream_decoder_destroy"
    KEYS = ("streams", "msgs", "rrs", "names", "tails", "counts")
    ASM_KEYS = TLSStreamDecoder.ASM_KEYS

    def __init__(self, max_streams=1, max_msgs=None, device=0):
        self.max_msgs = int(max_msgs if max_msgs is not None else max(4 * int(max_streams), 1024))
        if device is None:  # host-only: no handle
            self.h, self.max_packets = ctypes.c_void_p(), int(max_streams)
            return
        self.h = ctypes.c_void_p()
        _lib.check(_lib.lib().gpk_dns_stream_decoder_create(ctypes.byref(self.h), int(device), int(max_streams),
                                                            self.max_msgs))
        self.max_packets = int(max_streams)

    @staticmethod
    def needed(counts):
        """(message entries, rr entries, name bytes, tail bytes) the call needs, from counts[12]."""
        return tuple(int(x) for x in counts[5:9])

    @staticmethod
    def _structs(ptr, numel, asm, carry, caps, out, frame_unstarted, max_message):
        a = _lib.TcpStreams(*[ptr(asm[k]) if asm.get(k) is not None else None for k in DNSStreamDecoder.ASM_KEYS],
                            int(asm.get("chunk_cap", numel(asm["chunks"]) // _lib.TCP_CHUNK_DTYPE.itemsize)),
                            int(asm.get("data_cap", numel(asm["data"]))))
        flags = _lib.DNSS_FRAME_UNSTARTED if frame_unstarted else 0
        if carry is None:
            i = _lib.DnsStreamIn(None, None, None, None, 0, 0, flags, int(max_message))
        else:
            state, off, ln, tails = carry
            nt = 0 if tails is None else numel(tails)
            i = _lib.DnsStreamIn(ptr(state), ptr(off), ptr(ln), ptr(tails) if nt else None, numel(state), nt, flags,
                                 int(max_message))
        o = _lib.DnsStreamOut(ptr(out["streams"]), *[ptr(out[k]) if c else None for k, c in
                                                     zip(("msgs", "rrs", "names", "tails"), caps)],
                              ptr(out["counts"]), *caps)
        return a, i, o

    def decode(self, ctx, parser, data, offsets, caplens, records, layouts, asm, msg_cap, rr_cap, name_cap, tail_cap,
               carry=None, frame_unstarted=False, max_message=0, out=None, stream=None):
        """Device tensors in: the batch the assembler was given, its records
        and layouts, and `asm`, the dict Assembler.assemble returned for it.
        Returns dict(streams[64 n] (uint8, _lib.DNS_STREAM_DTYPE), msgs[80
        msg_cap] (uint8, _lib.DNS_STREAM_MSG_DTYPE), rrs[96 rr_cap],
        names[name_cap], tails[tail_cap], counts[12] (int64)) of device tensors
        (or fills `out`); stream entries at and past counts[0] are not written,
        nor is anything past a capacity. Asynchronous on `stream`."""
        import torch
        caps = (int(msg_cap), int(rr_cap), int(name_cap), int(tail_cap))
        n, dev = offsets.numel(), offsets.device
        if out is None:
            u8 = torch.uint8
            out = dict(streams=torch.empty(max(n, 1) * 64, dtype=u8, device=dev),
                       msgs=torch.empty(caps[0] * _lib.DNS_STREAM_MSG_DTYPE.itemsize, dtype=u8, device=dev),
                       rrs=torch.empty(caps[1] * _lib.DNS_RR_DTYPE.itemsize, dtype=u8, device=dev),
                       names=torch.empty(caps[2], dtype=u8, device=dev), tails=torch.empty(caps[3], dtype=u8, device=dev),
                       counts=torch.zeros(12, dtype=torch.int64, device=dev))
        a, i, o = self._structs(lambda t: t.data_ptr(), lambda t: t.numel(), asm, carry, caps, out, frame_unstarted,
                                max_message)
        b = _lib.Batch.of(data, offsets, caplens)
        r = _lib.Results(records.data_ptr(), None, None, layouts.data_ptr())
        _lib.check(_lib.lib().gpk_dns_streams(self.h, ctx.h, parser.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(a),
                                              ctypes.byref(i), ctypes.byref(o), _lib.stream_ptr(stream)))
        return out

    def decode_all(self, ctx, parser, data, offsets, caplens, records, layouts, asm, msg_cap=0, rr_cap=0, name_cap=0,
                   tail_cap=0, carry=None, frame_unstarted=False, max_message=0, stream=None):
        """decode with capacities that hold everything: a first call with the
        capacities given and, while counts reports an overflow, another with
        every capacity raised to what counts names: once for the streams'
        message entries and tails, once more for the messages' entries and
        names (at most three calls). Synchronizes on the counts. A call that
        needs more than max_msgs message entries raises."""
        caps = (int(msg_cap), int(rr_cap), int(name_cap), int(tail_cap))
        for _ in range(3):
            out = self.decode(ctx, parser, data, offsets, caplens, records, layouts, asm, *caps, carry=carry,
                              frame_unstarted=frame_unstarted, max_message=max_message, stream=stream)
            counts = out["counts"].cpu().tolist()
            if not counts[4]:
                break
            caps = tuple(max(c, x) for c, x in zip(caps, self.needed(counts)))
        return out

    @classmethod
    def decode_host(cls, parser, data, offsets, caplens, records, layouts, asm, msg_cap, rr_cap, name_cap, tail_cap,
                    carry=None, frame_unstarted=False, max_message=0, fill=0):
        """The same over numpy arrays on the calling thread
        (gpk_dns_streams_host); asm holds the assembler's outputs as numpy
        arrays (chunks as _lib.TCP_CHUNK_DTYPE, stream_first, stream_closed,
        stream_data0, counts, data at least); `fill` is the byte the outputs
        start with."""
        import numpy as np
        caps = (int(msg_cap), int(rr_cap), int(name_cap), int(tail_cap))
        keep = (np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(offsets, np.uint64),
                np.ascontiguousarray(caplens, np.uint32), np.ascontiguousarray(records, _lib.RECORD_DTYPE),
                np.ascontiguousarray(layouts, _lib.LAYOUT_DTYPE))
        n = len(keep[2])
        asm = dict(asm)
        for k, dt in (("chunks", _lib.TCP_CHUNK_DTYPE), ("stream_first", np.uint32), ("stream_closed", np.uint32),
                      ("stream_data0", np.uint64), ("counts", np.uint64), ("data", np.uint8)):
            asm[k] = np.ascontiguousarray(asm[k], dt)
        asm.setdefault("chunk_cap", len(asm["chunks"]))
        asm.setdefault("data_cap", len(asm["data"]))
        if carry is not None:
            carry = (np.ascontiguousarray(carry[0], np.uint32), np.ascontiguousarray(carry[1], np.uint64),
                     np.ascontiguousarray(carry[2], np.uint32),
                     None if carry[3] is None else np.ascontiguousarray(carry[3], np.uint8))
        out = dict(streams=np.empty(max(n, 1), _lib.DNS_STREAM_DTYPE), msgs=np.empty(caps[0], _lib.DNS_STREAM_MSG_DTYPE),
                   rrs=np.empty(caps[1], _lib.DNS_RR_DTYPE), names=np.empty(caps[2], np.uint8),
                   tails=np.empty(caps[3], np.uint8), counts=np.empty(12, np.uint64))
        for v in out.values():
            v.view(np.uint8)[:] = fill
        a, i, o = cls._structs(lambda t: t.ctypes.data, lambda t: t.size, asm, carry, caps, out, frame_unstarted,
                               max_message)
        b = _lib.Batch(keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, n, keep[0].size)
        r = _lib.Results(keep[3].ctypes.data, None, None, keep[4].ctypes.data)
        _lib.check(_lib.lib().gpk_dns_streams_host(parser.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(a),
                                                   ctypes.byref(i), ctypes.byref(o)))
        return out

    @classmethod
    def decode_host_all(cls, parser, data, offsets, caplens, records, layouts, asm, msg_cap=0, rr_cap=0, name_cap=0,
                        tail_cap=0, carry=None, frame_unstarted=False, max_message=0):
        """decode_host with the retries of decode_all."""
        caps = (int(msg_cap), int(rr_cap), int(name_cap), int(tail_cap))
        for _ in range(3):
            out = cls.decode_host(parser, data, offsets, caplens, records, layouts, asm, *caps, carry=carry,
                                  frame_unstarted=frame_unstarted, max_message=max_message)
            if not int(out["counts"][4]):
                break
            caps = tuple(max(c, x) for c, x in zip(caps, cls.needed(out["counts"])))
        return out


class DNSStreamResult:
    """What DNSStreams returns for one call. streams: [dict(id (global), state
    (DNSS_*), status, tail_in, msgs (DNS_STREAM_MSG_DTYPE), closed, and key
    with keys=True on a new stream)]; offsets of msgs and of their entries are
    relative to the stream's logical buffer of this call (tail_in carried
    bytes, then the new ones). counts: gpk_dns_stream_out.counts. rrs and names
    are the call's arenas on the host. The streams' bytes stay on the device
    until messages() asks for the logical buffers of the streams that have
    decoded messages."""

    def __init__(self, streams, counts, assembled, rrs=None, names=None, buffers=None):
        self.streams, self.counts, self.assembled = streams, counts, assembled
        self.rrs, self.names, self._buffers, self._bytes = rrs, names, buffers, None

    @staticmethod
    def _decoded(m):
        return not int(m["status"]) and not int(m["msg"]["err"])

    def _logical(self):
        """{stream index: its logical buffer} for the streams with decoded messages: one device gather, one copy."""
        if self._bytes is None:
            import torch
            self._bytes = {}
            want = [j for j, s in enumerate(self.streams) if any(self._decoded(m) for m in s["msgs"])]
            if want:
                parts = [p for j in want for p in self._buffers(j)]
                flat = torch.cat(parts).cpu().numpy().tobytes() if parts else b""
                at = 0
                for j in want:
                    n = sum(p.numel() for p in self._buffers(j))
                    self._bytes[j] = flat[at:at + n]
                    at += n
        return self._bytes

    def messages(self):
        """[(global stream id, layers.DNS)] of the messages that decoded, in stream and message order."""
        from . import layers
        out, bufs = [], self._logical()
        for j, s in enumerate(self.streams):
            for m in s["msgs"]:
                if self._decoded(m):
                    t = m["msg"]
                    d = layers.DNS()
                    d._from_record(t, self.rrs[int(t["rr0"]):int(t["rr0"]) + int(t["nrr"])], self.names, bufs[j])
                    out.append((s["id"], d))
        return out

    def questions(self):
        """[(global stream id, name, type)] of every question of the messages that decoded: from the tables and
        the names alone, no stream byte."""
        out = []
        for s in self.streams:
            for m in s["msgs"]:
                if self._decoded(m):
                    t = m["msg"]
                    for r in self.rrs[int(t["rr0"]):int(t["rr0"]) + int(t["qdcount"])]:
                        o = int(r["name_off"])
                        out.append((s["id"], bytes(self.names[o:o + int(r["name_len"])]), int(r["type"])))
        return out


class DNSStreams(_StreamPass):
    """DNS over reassembled streams: a TCPAssembler and a DNSStreamDecoder
    behind it, over a stream of device batches; state and tails are carried as
    _StreamPass describes. max_message (0: none) is gpk_dns_stream_in's
    max_msg_len, the work cap for untrusted traffic: longer messages are framed
    over and come back as DNSS_MSG_SKIPPED. The capacities a call needed are
    kept as the first guess of the next, and the decoder grows with the number
    of messages a call holds."""
    _NEW = _lib.DNSS_NEW

    def __init__(self, ctx, parser, max_packets, max_pages=0, timed=False, frame_unstarted=False, max_message=0,
                 device=0, keys=False):
        self.max_message = int(max_message)
        self._max_msgs = max(4 * int(max_packets), 1024)
        self._caps = (0, 0, 0, 0)
        super().__init__(ctx, parser, max_packets, max_pages=max_pages, timed=timed, frame_unstarted=frame_unstarted,
                         device=device, keys=keys)

    def _new_decoder(self):
        return DNSStreamDecoder(self.asm.max_packets, self._max_msgs, self.device)

    def _decode(self, res):
        if self.asm._last is None or not res["streams"]:
            return DNSStreamResult([], [0] * 12, res)
        last, carry = self._carry_in()
        ids = last["ids"]
        S = len(ids)
        caps = tuple(min(c, m) for c, m in zip(self._caps, (self._max_msgs,) + (1 << 62,) * 3))
        for _ in range(4):
            out = self.decoder.decode(self.ctx, self.parser, last["data"], last["offsets"], last["caplens"],
                                      last["records"], last["layouts"], last["out"], *caps, carry=carry,
                                      frame_unstarted=self.frame_unstarted, max_message=self.max_message,
                                      stream=last["stream"])
            counts = out["counts"].cpu().tolist()
            if not counts[4]:
                break
            need = DNSStreamDecoder.needed(counts)
            if need[0] > self._max_msgs:  # more messages than the decoder's scans hold
                self._max_msgs = 2 * need[0]
                self.decoder.close()
                self.decoder = self._new_decoder()
            caps = tuple(max(c, x) for c, x in zip(caps, need))
        self._caps = caps
        self._last_call = dict(carry=carry, out=out, caps=caps)  # what went in beside asm._last, and what came out
        ent = out["streams"].cpu().numpy().view(_lib.DNS_STREAM_DTYPE)[:S]
        msgs = out["msgs"].cpu().numpy().view(_lib.DNS_STREAM_MSG_DTYPE)
        rrs = out["rrs"].cpu().numpy().view(_lib.DNS_RR_DTYPE)
        names = out["names"].cpu().numpy()
        streams = []
        for g, e, a in zip(ids, ent, res["streams"]):
            m0 = int(e["msg0"])
            d = dict(id=g, state=int(e["state"]), status=int(e["status"]), tail_in=int(e["tail_in"]),
                     msgs=msgs[m0:m0 + int(e["nmsg"])], closed=a["closed"])
            if "key" in a:
                d["key"] = a["key"]
            streams.append(d)
        tails_in, toff = carry[3], carry[1].cpu().tolist()
        data = last["out"]["data"]

        def buffers(j):  # the device slices of stream j's logical buffer
            a, t = res["streams"][j], streams[j]["tail_in"]
            return ([tails_in[toff[j]:toff[j] + t]] if t else []) + [data[a["data0"]:a["data1"]]]
        self._carry_out(ids, ent, res["streams"], out["tails"])
        return DNSStreamResult(streams, counts, res, rrs, names, buffers)
