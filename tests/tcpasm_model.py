"""Pure-Python restatement of tcpassembly's reassembly (tcpassembly/assembly.go),
quirks included. TEST INFRASTRUCTURE ONLY: the checker of
gopacket_amd/csrc/gpk_tcpasm.hip (include/gpk_tcpasm.h).

Input: the packets, the decode oracle's records and layouts, and
oracle/flows_oracle.py's CONNECTION keying (the "useless packet" filter, :538).
One run behaves like a fresh NewAssembler(NewStreamPool(factory)) with
MaxBufferedPagesPerConnection = max_pages and MaxBufferedPagesTotal = 0, fed the
keyed packets in order through AssembleWithTimestamp, then FlushAll() if asked.

  - Sequence.Difference (:57-64) in unbounded ints with the quarter-space rule
    as written; Add masks to 32 bits (:67-69); invalidSequence = -1
  - getConnection(key, end = !SYN && len(payload) == 0) creates nothing for a
    bare FIN/RST on a key with no open connection (:552-566)
  - first SYN on an invalid nextSeq: Start, the whole payload, seq+len+1 (:571-582)
  - byteSpan (:612-623), its `len(bytes) < span` case included: empty bytes,
    nextSeq unchanged
  - sendToConnection closes only on the LAST element's End (:627-636)
  - pagesFromTCP: pages of 1900, an empty payload makes one, End on the last
    (:737-759); traverseConn scans from the back (:686-693); the page limit pops
    ONE page (:723-729); addNextFromConn's Skip (:763-783)
  - FlushAll: skipFlush until closed (:279-290, :648-660)
  - the panic("wtf") of insertIntoConn (:716-718) raises Wtf

Seen, lastSeen, FlushOlderThan are not modelled: a chunk names its source packet.
The payload of a packet is tcp[min(DataOffset*4, len) :] of the layout's TCP
slice (empty where the header claims more than the slice holds).
"""
from oracle import flows_oracle as FO

DIRECT, QUEUED, NOCONN, CARRIED, EBADCARRY, EPANIC = -24, -25, -26, -27, -28, -29
START, END = 1, 2
CALL_FLUSH = 1 << 31
OPEN = 0xFFFFFFFF
NO_CONN = -2
CARRY_CONN = 1 << 31
CARRY_PAGE = 1 << 30
PAGE_BYTES = 1900
U32 = 1 << 32
INVALID = -1
SLOT_TCP = FO.SLOT_TCP


class Wtf(Exception):
    """insertIntoConn's panic("wtf") (:716-718)"""


def difference(s, t):
    """Sequence.Difference (:57-64)"""
    if s > U32 - U32 // 4 and t < U32 // 4:
        t += U32
    elif t > U32 - U32 // 4 and s < U32 // 4:
        s += U32
    return t - s


def add(s, t):
    return (s + t) & (U32 - 1)


def byte_span(expected, received, off, length):
    """byteSpan (:612-623) on a slice (off, length) of the source payload -> (off, length, next)"""
    if expected == INVALID:
        return off, length, add(received, length)
    span = difference(received, expected)
    if span <= 0:
        return off, length, add(received, length)
    if length < span:
        return off + length, 0, expected
    return off + span, length - span, add(expected, length - span)


class Seg:
    __slots__ = ("idx", "seq", "syn", "end", "plen", "pstart")

    def __init__(self, idx, pkt, lay):
        t0, t1 = int(lay["start"][SLOT_TCP]), int(lay["end"][SLOT_TCP])
        tcp = pkt[t0:t1]
        hdr = min((tcp[12] >> 4) * 4, len(tcp))
        self.idx, self.seq = idx, int.from_bytes(tcp[4:8], "big")
        self.syn, self.end = bool(tcp[13] & 2), bool(tcp[13] & 5)
        self.plen, self.pstart = len(tcp) - hdr, t0 + hdr

    def pages(self):
        return max(1, -(-self.plen // PAGE_BYTES))

    def page(self, k):
        """pagesFromTCP's page k: (seq, off, length, End)"""
        n = self.pages()
        ln = min(PAGE_BYTES, self.plen - PAGE_BYTES * k)
        return [add(self.seq, PAGE_BYTES * k), PAGE_BYTES * k, ln, self.end and k == n - 1, self.idx, k]


class Conn:
    def __init__(self, stream, next_seq=INVALID):
        self.stream, self.next_seq, self.pages = stream, next_seq, []


class Model:
    def __init__(self, max_pages):
        self.max_pages = max_pages
        self.streams, self.log, self.ret = [], [], []

    def new_stream(self, group, first):
        self.streams.append(dict(group=group, first=first, closed=OPEN, chunks=[]))
        self.log.append(("New", len(self.streams) - 1))
        return len(self.streams) - 1

    def chunk(self, src, off, ln, skip, flags):
        self.ret.append(dict(src=src, src_off=off, len=ln, skip=skip, flags=flags))

    def add_next(self, c):
        """addNextFromConn (:763-783)"""
        seq, off, ln, end, src, _ = c.pages.pop(0)
        skip = 0
        if c.next_seq == INVALID:
            skip = -1
        else:
            d = difference(c.next_seq, seq)
            if d > 0:
                skip = d
        off, ln, c.next_seq = byte_span(c.next_seq, seq, off, ln)
        self.chunk(src, off, ln, skip, END if end else 0)

    def add_contiguous(self, c):
        """:639-643"""
        while c.pages and difference(c.next_seq, c.pages[0][0]) <= 0:
            self.add_next(c)

    def send(self, c, call):
        """sendToConnection (:627-636) -> closed"""
        self.add_contiguous(c)
        st = self.streams[c.stream]
        for r in self.ret:
            r["call"] = call
        st["chunks"] += self.ret
        self.log.append(("Reassembled", c.stream, call, len(self.ret)))
        closed = bool(self.ret[-1]["flags"] & END)
        self.ret = []
        if closed:
            self.close(c, call)
        return closed

    def close(self, c, call):
        self.streams[c.stream]["closed"] = call
        self.log.append(("ReassemblyComplete", c.stream, call))

    def insert(self, c, s):
        """insertIntoConn (:715-730)"""
        if c.pages and c.pages[0][0] == c.next_seq:
            raise Wtf(s.idx)
        new = [s.page(k) for k in range(s.pages())]
        at = len(c.pages)  # traverseConn: from the back
        while at > 0 and difference(c.pages[at - 1][0], s.seq) < 0:
            at -= 1
        c.pages[at:at] = new
        if self.max_pages > 0 and len(c.pages) >= self.max_pages:
            self.add_next(c)

    def assemble(self, c, s):
        """AssembleWithTimestamp from :570 -> (verdict, closed)"""
        self.ret = []
        direct = True
        if c.next_seq == INVALID:
            if s.syn:
                self.chunk(s.idx, 0, s.plen, 0, START)
                c.next_seq = add(s.seq, s.plen + 1)
            else:
                direct = False
        elif difference(c.next_seq, s.seq) > 0:
            direct = False
        else:
            off, ln, c.next_seq = byte_span(c.next_seq, s.seq, 0, s.plen)
            self.chunk(s.idx, off, ln, 0, END if s.end else 0)
        if not direct:
            self.insert(c, s)
        closed = self.send(c, s.idx) if self.ret else False
        return (DIRECT if direct else QUEUED), closed


def run(packets, records, layouts, max_pages=0, flush=False, carry=()):
    """carry: [(code, seq)] for the first len(carry) packets (include/gpk_tcpasm.h).
    -> dict(verdict, stream_of, streams: [dict(group, first, closed, chunks, data)],
    conn_seq, conn_stream (per group), pend: [(packet, page)], counts, log)."""
    m = Model(max_pages)
    groups, conns, verdict, stream_of = {}, {}, [], []
    for i, pkt in enumerate(packets):
        k = FO.packet_key(FO.CONNECTION, pkt, records[i], layouts[i], 0, 8)
        if isinstance(k, int):
            verdict.append(k)
            stream_of.append(-1)
            continue
        g = groups.setdefault(k, len(groups))
        s = Seg(i, pkt, layouts[i])
        c = conns.get(g)
        if i < len(carry):
            code, seq = carry[i]
            if code & CARRY_CONN and not code & CARRY_PAGE and c is None:
                conns[g] = Conn(m.new_stream(g, i), seq)
                verdict.append(CARRIED)
                stream_of.append(conns[g].stream)
            elif code & CARRY_PAGE and not code & CARRY_CONN and c is not None and (code & 0xFFFF) < s.pages():
                c.pages.append(s.page(code & 0xFFFF))
                verdict.append(CARRIED)
                stream_of.append(c.stream)
            else:
                verdict.append(EBADCARRY)
                stream_of.append(-1)
            continue
        if c is None:
            if not s.syn and s.plen == 0:  # getConnection(key, end=true) (:552-560)
                verdict.append(NOCONN)
                stream_of.append(-1)
                continue
            c = conns[g] = Conn(m.new_stream(g, i))
        v, closed = m.assemble(c, s)
        verdict.append(v)
        stream_of.append(c.stream)
        if closed:
            del conns[g]
    if flush:  # FlushAll (:279-290): skipFlush (:648-660) until closed
        for g in sorted(conns, key=lambda g: conns[g].stream):
            c, rnd = conns[g], 0
            while True:
                call = CALL_FLUSH | rnd
                rnd += 1
                if not c.pages:
                    m.close(c, call)
                    break
                m.ret = []
                m.add_next(c)
                if m.send(c, call):
                    break
        conns = {}
    G = len(groups)
    conn_seq, conn_stream = [NO_CONN] * G, [-1] * G
    pend = []
    for g in sorted(conns):
        conn_seq[g], conn_stream[g] = conns[g].next_seq, conns[g].stream
        pend += [(p[4], p[5]) for p in conns[g].pages]
    nbytes = 0
    for st in m.streams:
        parts = []
        for ch in st["chunks"]:
            sg = Seg(ch["src"], packets[ch["src"]], layouts[ch["src"]])
            parts.append(bytes(packets[ch["src"]][sg.pstart + ch["src_off"]:sg.pstart + ch["src_off"] + ch["len"]]))
            assert len(parts[-1]) == ch["len"]
        st["data"] = b"".join(parts)
        nbytes += len(st["data"])
    nchunks = sum(len(st["chunks"]) for st in m.streams)
    return dict(verdict=verdict, stream_of=stream_of, streams=m.streams, conn_seq=conn_seq, conn_stream=conn_stream,
                pend=pend, log=m.log, groups=G,
                counts=[len(m.streams), nchunks, nbytes, len(pend), len(conns), 0, 0, 0])
