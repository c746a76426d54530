"""Time in the two fragment reassemblers, restated sequentially on top of the
untimed models (tests/defrag_model.py, tests/defrag6_model.py, imported
unchanged): per-packet timestamps plus a program of DiscardOlderThan calls at
packet positions. TEST INFRASTRUCTURE ONLY: the checker of
gpk_defrag_batch_timed and gpk_defrag6_batch_timed and of the timed streaming
classes of gopacket_amd.flows.

Timestamps are int64 nanoseconds (time.Time.UnixNano()); Before is <.

IPv4 (ip4defrag/defrag.go): fragmentList.LastSeen = t (:249) is an assignment
made by every insert that passes the duplicate check (counted-not-listed
fragments and fragments whose build fails included); an ignored duplicate
(:223-238) returns before it; a call that fails the security checks never gets
there. DiscardOlderThan(t) (:138-149) deletes the keys with LastSeen < t and
returns how many.

IPv6 (ip6defrag/defrag.go): the deferred d.container[id].time = time.Now()
(:84-87) stamps the key's head entry after every call on the Identification;
DiscardOlderThan (:183-194) reads the head entry's time. The model keeps the
time per entry object exactly so, and asserts that it equals the timestamp
of the key's last call. The caller's timestamp plays time.Now().

ops: [(position, t)], DiscardOlderThan(t) before the packet at `position`
(position == len(packets): after the last one), in list order.
"""
import defrag6_model as M6
import defrag_model as M4
from oracle import flows_oracle as FO


def _ops_at(ops, n):
    at = {}
    for pos, t in ops:
        assert 0 <= pos <= n
        at.setdefault(pos, []).append(t)
    return at


def run4(packets, records, layouts, seen, ops=()):
    """-> dict(verdict, datagrams (as defrag_model.run), pending, pending_seen
    (LastSeen of each pending packet's key), last_seen: key -> LastSeen,
    discards: per op (keys discarded, packets dropped with them), in ops order)."""
    flows, last_seen, verdict, datagrams, discards = {}, {}, [], [], []
    at = _ops_at(ops, len(packets))

    def discard(t):
        old = [k for k in flows if last_seen[k] < t]
        discards.append((len(old), sum(len(flows[k].counted) for k in old)))
        for k in old:
            del flows[k], last_seen[k]

    for i, pkt in enumerate(packets):
        for t in at.get(i, ()):
            discard(t)
        k = FO.packet_key(FO.DEFRAG, pkt, records[i], layouts[i], 0, 8)
        if isinstance(k, int):
            verdict.append(k)
            continue
        f = M4.Frag(i, pkt, layouts[i])
        fl = flows.setdefault(k, M4.FragList())
        before = len(fl.counted)
        out, v = fl.insert(f)
        if len(fl.counted) != before:  # past the duplicate check: f.LastSeen = t
            last_seen[k] = seen[i]
        if out is None and len(fl.list) + 1 > M4.MAX_LIST:
            del flows[k], last_seen[k]
            v = M4.EMAXLEN
        if out is not None:
            v = len(datagrams)
            datagrams.append(dict(last=i, length=fl.highest, payload=out, payload_off=f.start + f.ihl * 4,
                                  data=M4.datagram_bytes(pkt, f, out)))
            del flows[k], last_seen[k]
        verdict.append(v)
    for t in at.get(len(packets), ()):
        discard(t)
    assert set(flows) == set(last_seen)
    for k, fl in flows.items():  # the identity the device relies on
        assert fl.counted and last_seen[k] == seen[fl.counted[-1]]
    key_of = {i: k for k, fl in flows.items() for i in fl.counted}
    pending = sorted(key_of)
    return dict(verdict=verdict, datagrams=datagrams, pending=pending,
                pending_seen=[last_seen[key_of[i]] for i in pending], last_seen=dict(last_seen), discards=discards)


def run6(packets, records, layouts, seen, ops=(), carry=0):
    """-> dict(verdict, datagrams (as defrag6_model.run), pending (listed
    fragments of the live keys), pending_seen, key_time: Identification -> time,
    discards: per op (keys discarded, listed fragments dropped with them))."""
    d = M6.IPv6Defragmenter()
    verdict, datagrams, discards = [], [], []
    listed, last_call = {}, {}  # per live key: its listed packets; the timestamp of its last call
    etime = {}  # fragment.time, per entry object (the untimed model's entries have no such field)
    at = _ops_at(ops, len(packets))

    def discard(t):
        old = [k for k, v in d.container.items() if etime[id(v)] < t]
        discards.append((len(old), sum(len(listed[k]) for k in old)))
        for k in old:
            del d.container[k], listed[k], last_call[k]

    for i, pkt in enumerate(packets):
        for t in at.get(i, ()):
            discard(t)
        f = M6.find_fragment(pkt, layouts[i])
        if f is None:
            verdict.append(M6.NONE)
            continue
        s, a, end = f
        fg = M6.fragment_layer(pkt, a, end)
        out = d.DefragIPv6(M6.ipv6_layer(pkt, s), fg, tag=(i, s))
        etime[id(d.container[fg.Identification])] = seen[i]  # the deferred stamp, on the head entry as it is now
        last_call[fg.Identification] = seen[i]
        if d.listed:
            listed.setdefault(fg.Identification, []).append(i)
        if i < carry:
            verdict.append(M6.CARRIED)
        elif out is None:
            verdict.append(M6.HELD)
        else:
            hp, hs = out.head
            verdict.append(len(datagrams))
            datagrams.append(dict(last=i, head=hp, length=len(out.Payload), nextheader=out.NextHeader,
                                  payload=out.Payload, payload_off=hs + 40,
                                  data=M6.datagram_bytes(packets[hp], hs, out), layer=out))
    for t in at.get(len(packets), ()):
        discard(t)
    key_time = {k: etime[id(v)] for k, v in d.container.items()}
    assert key_time == last_call  # a key's time is the timestamp of its last call
    key_of = {i: k for k, v in listed.items() for i in v}
    pending = sorted(key_of)
    return dict(verdict=verdict, datagrams=datagrams, pending=pending,
                pending_seen=[key_time[key_of[i]] for i in pending], key_time=key_time, discards=discards)
