"""Time in tcpassembly (tcpassembly/assembly.go), restated sequentially on top
of the untimed model (tests/tcpasm_model.py, imported unchanged): per-packet
timestamps plus a program of FlushWithOptions calls at packet positions. TEST
INFRASTRUCTURE ONLY: the checker of gpk_tcpasm_batch_timed and of the timed
flows.TCPAssembler / tcpassembly.Assembler.

Timestamps are int64 nanoseconds (time.Time.UnixNano()); Before is <; Go's zero
time.Time is ZERO = INT64_MIN.

  - lastSeen (:567-569): every call that gets a connection does
    if lastSeen.Before(ts) lastSeen = ts, a maximum. "Useless" packets (:538)
    and calls that get no connection (:555) never reach it.
  - page.Seen is the timestamp of the page's source packet.
  - FlushWithOptions (:238-269): per connection, while the list is not empty and
    the FIRST page's Seen < T: skipFlush; a send that closed ends the loop. With
    CloseAll a connection still open, drained and with lastSeen < T is closed.
    The reference visits connections in a Go map's order; here stream order.
  - recycle: the reference's free list. connection.reset (:388-396) keeps
    lastSeen and StreamPool hands out structs LIFO (grow: initialAllocSize 1024,
    doubling, :324-334; newConnection pops the last, :489-490; remove appends,
    :665), so a new connection inherits the lastSeen of the closed connection
    that last used its struct. recycle=False is the device's rule: every new
    connection starts from ZERO.

ops: [(position, t, close_all)], FlushWithOptions{T: t, CloseAll: close_all}
before the packet at `position` (len(packets): after the last one). A flush
call is ("flush", op number, round).
"""
import tcpasm_model as M
from oracle import flows_oracle as FO

ZERO = -(1 << 63)
INITIAL_ALLOC = 1024


class Struct:
    """the part of a connection struct that outlives reset"""

    def __init__(self):
        self.last_seen = ZERO


class Pool:
    def __init__(self, recycle):
        self.recycle, self.free, self.next_alloc = recycle, [], INITIAL_ALLOC

    def get(self):
        if not self.recycle:
            return Struct()
        if not self.free:
            self.free += [Struct() for _ in range(self.next_alloc)]
            self.next_alloc *= 2
        return self.free.pop()

    def put(self, s):
        if self.recycle:
            self.free.append(s)


def run(packets, records, layouts, seen, ops=(), max_pages=0, recycle=False):
    """-> tcpasm_model.run's dict (chunks also carry `seen`), plus
    conn_last_seen (per group, ZERO where no connection is open), pend_seen
    (per pending page), flushes: per op (flushed, closed), and events: per op
    {stream: what happened to it}, one of "untouched", "shielded" (left alone
    behind a young first page though an older page is listed), "flushed",
    "closed by End", "closed by CloseAll"."""
    m = M.Model(max_pages)
    pool = Pool(recycle)
    groups, conns, verdict, stream_of, flushes, events = {}, {}, [], [], [], []
    at = {}
    for k, (pos, t, close_all) in enumerate(ops):
        assert 0 <= pos <= len(packets)
        at.setdefault(pos, []).append((k, t, close_all))

    def drop(g):
        pool.put(conns[g].box)
        del conns[g]

    def flush(k, t, close_all):
        nf = nc = 0
        ev = {}
        for g in sorted(conns, key=lambda g: conns[g].stream):
            c, rnd, did, shut = conns[g], 0, False, None
            shielded = bool(c.pages) and seen[c.pages[0][4]] >= t and any(seen[p[4]] < t for p in c.pages)
            while c.pages and seen[c.pages[0][4]] < t:
                call = ("flush", k, rnd)
                rnd += 1
                m.ret = []
                m.add_next(c)  # skipFlush (:648-660)
                did = True
                if m.send(c, call):
                    shut = "closed by End"
                    break
            if close_all and shut is None and not c.pages and c.box.last_seen < t:
                m.close(c, ("flush", k, rnd))
                did, shut = True, "closed by CloseAll"
            nf += did
            nc += shut is not None
            ev[c.stream] = shut or ("flushed" if did else "shielded" if shielded else "untouched")
            if shut:
                drop(g)
        flushes.append((nf, nc))
        events.append(ev)

    for i, pkt in enumerate(packets):
        for op in at.get(i, ()):
            flush(*op)
        k = FO.packet_key(FO.CONNECTION, pkt, records[i], layouts[i], 0, 8)
        if isinstance(k, int):
            verdict.append(k)
            stream_of.append(-1)
            continue
        g = groups.setdefault(k, len(groups))
        s = M.Seg(i, pkt, layouts[i])
        c = conns.get(g)
        if c is None:
            if not s.syn and s.plen == 0:
                verdict.append(M.NOCONN)
                stream_of.append(-1)
                continue
            c = conns[g] = M.Conn(m.new_stream(g, i))
            c.box = pool.get()
        if c.box.last_seen < seen[i]:
            c.box.last_seen = seen[i]
        v, closed = m.assemble(c, s)
        verdict.append(v)
        stream_of.append(c.stream)
        if closed:
            drop(g)
    for op in at.get(len(packets), ()):
        flush(*op)
    G = len(groups)
    conn_seq, conn_stream, conn_last_seen = [M.NO_CONN] * G, [-1] * G, [ZERO] * G
    pend = []
    for g in sorted(conns):
        conn_seq[g], conn_stream[g], conn_last_seen[g] = conns[g].next_seq, conns[g].stream, conns[g].box.last_seen
        pend += [(p[4], p[5]) for p in conns[g].pages]
    nbytes = 0
    for st in m.streams:
        parts = []
        for ch in st["chunks"]:
            sg = M.Seg(ch["src"], packets[ch["src"]], layouts[ch["src"]])
            parts.append(bytes(packets[ch["src"]][sg.pstart + ch["src_off"]:sg.pstart + ch["src_off"] + ch["len"]]))
            ch["seen"] = seen[ch["src"]]
        st["data"] = b"".join(parts)
        nbytes += len(st["data"])
    nchunks = sum(len(st["chunks"]) for st in m.streams)
    return dict(verdict=verdict, stream_of=stream_of, streams=m.streams, conn_seq=conn_seq, conn_stream=conn_stream,
                conn_last_seen=conn_last_seen, pend=pend, pend_seen=[seen[p] for p, _ in pend], log=m.log, groups=G,
                flushes=flushes, events=events,
                counts=[len(m.streams), nchunks, nbytes, len(pend), len(conns), 0, 0, 0])
