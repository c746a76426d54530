"""Packets for the TLS-over-streams tests (include/gpk_tls_streams.h): TCP
connections that carry TLS records cut into segments, built with tcpasmcases.seg
and the record builders of tlscases.

A case is dict(name, calls=[[packet, ...], ...], max_pages, frame_unstarted,
flush): the calls are fed in order and, with flush, a FlushAll follows.
"""
import random

import tcpasmcases as TC
import tlscases as C
from tlscases import ALERT, APP, CCS, HS, hello, hs_body, rec, sni_ext

PARSER = C.PARSER
SYN, FIN = TC.SYN, TC.FIN
MSS = 1448


def addr(i):
    """Source address and port of connection i: distinct keys for any number of connections."""
    return (10, (i >> 24) & 255 or 1, (i >> 16) & 255, (i >> 8) & 255), 1024 + (i & 255) * 97 % 60000 + (i & 255)


def cut(payload, cuts):
    """payload cut at the positions `cuts` (sorted) -> [(offset, bytes)]"""
    edges = [0] + [c for c in cuts if 0 < c < len(payload)] + [len(payload)]
    return [(a, payload[a:b]) for a, b in zip(edges, edges[1:])]


def conn(i, payload, cuts=(), dport=443, sport=None, isn=1000, syn=True, fin=False, drop=(), order=None):
    """The frames of connection i in one direction: SYN, the payload cut at
    `cuts`, FIN. drop: segment numbers left out; order: a permutation of the
    data segments."""
    src, sp = addr(i)
    sp = sp if sport is None else sport
    kw = dict(src=src, sport=sp, dport=dport)
    out = [TC.seg(isn, SYN, **kw)] if syn else []
    segs = [TC.seg(isn + 1 + at, 0, b, **kw) for k, (at, b) in enumerate(cut(payload, cuts)) if k not in drop]
    if order is not None:
        segs = [segs[k] for k in order]
    out += segs
    if fin:
        out.append(TC.seg(isn + 1 + len(payload), FIN, **kw))
    return out


def hello_rec(name=b"split.example", pad=120):
    """A ClientHello record of about 250 bytes with a server name."""
    return rec(HS, hello(sni_ext(name) + C.ext(21, bytes(pad)) + C.ALPN + C.GROUPS))


def flight(name=b"split.example"):
    """A ClientHello record, a CCS and an application record."""
    return hello_rec(name) + rec(CCS, b"\x01") + rec(APP, bytes(range(40)))


def split_streams(two_calls):
    """One stream per byte position of flight(): the payload in two segments cut
    there. -> calls"""
    msg = flight()
    a, b = [], []
    for k in range(1, len(msg)):
        fr = conn(k, msg, [k])
        a += fr[:2]
        (b if two_calls else a).append(fr[2])
    return [a, b] if two_calls else [a]


def largest():
    """One record of Length 65535 over 46 segments and three calls, then a small one."""
    msg = rec(APP, bytes((7 * k) & 255 for k in range(65535))) + rec(ALERT, b"\x01\x00")
    # the second call ends one byte short of the record: the tail peaks at 65539 bytes
    fr = conn(1, msg, [MSS * k for k in range(1, 45)] + [65539])
    assert len(fr) == 1 + 46
    return [fr[:21], fr[21:46], fr[46:]]


def quirk_streams():
    """Every hand-built message of tlscases as the whole payload of its own
    connection, closed by a FIN: the per-record failures, the terminal entries
    and the buffer that ends with the record."""
    out = []
    for i, (nm, pkt) in enumerate(C.quirk_cases()[0]):
        if pkt[12:14] != b"\x08\x00" or pkt[23] != 6:
            continue
        dport = int.from_bytes(pkt[36:38], "big")
        sport = int.from_bytes(pkt[34:36], "big")
        out += conn(i, pkt[C.AT:], [7], dport=dport, sport=443 if sport == 443 else None, fin=True)
    return out


def cases():
    c = []

    def add(name, calls, max_pages=0, frame_unstarted=False, flush=False):
        c.append(dict(name=name, calls=calls, max_pages=max_pages, frame_unstarted=frame_unstarted, flush=flush))
    add("split_one_call", split_streams(False))
    add("split_two_calls", split_streams(True))
    add("largest_record", largest())
    msg = flight(b"order.example") + rec(APP, bytes(500))
    cuts = [50, 120, 200, 260, 300, 500]
    add("out_of_order", [conn(1, msg, cuts, order=[2, 0, 1, 4, 3, 6, 5])])
    src, sp = addr(2)
    kw = dict(src=src, sport=sp, dport=443)
    add("overlap_and_retransmission", [[TC.seg(1000, SYN, **kw), TC.seg(1001, 0, msg[:100], **kw),
                                        TC.seg(1051, 0, msg[50:180], **kw), TC.seg(1001, 0, msg[:100], **kw),
                                        TC.seg(1181, 0, msg[180:], **kw), TC.seg(1001 + len(msg), FIN, **kw)]])
    # the page limit pops a page behind a hole: Skip > 0 without a close; what comes later is ignored
    many = flight(b"skip.example") + rec(APP, bytes(300)) * 4
    add("page_limit_forces_a_skip", [conn(3, many, [100, 300, 400, 600, 800, 1000], drop=(2,)),
                                     [TC.seg(1001 + len(many), 0, rec(APP, b"late"), src=addr(3)[0], sport=addr(3)[1],
                                             dport=443)]], max_pages=3)
    add("lost_middle_segment", [conn(4, many, [100, 300, 420], drop=(2,))], flush=True)
    add("fin_inside_a_record", [conn(5, flight() + rec(APP, bytes(100))[:60], [80], fin=True) +
                                conn(6, flight() + b"\x17\x03", [80], fin=True)])
    add("no_syn", [conn(7, flight(b"nosyn.example"), [90], syn=False)], flush=True)
    add("no_syn_framed", [conn(7, flight(b"nosyn.example"), [90], syn=False)], frame_unstarted=True, flush=True)
    add("not_tls_is_sticky", [conn(8, rec(APP, b"one") + rec(APP, b"two") + b"GET / HTTP/1.1\r\n" + rec(APP, b"x"), [9]),
                              [TC.seg(1001 + 48, 0, rec(APP, b"more"), src=addr(8)[0], sport=addr(8)[1], dport=443)]])
    add("server_direction", [conn(9, rec(HS, hs_body(2, 60)) + rec(CCS, b"\x01") + rec(APP, b"reply"), [30], dport=50000,
                                  sport=443)])
    add("host_name_panic", [conn(10, rec(APP, b"x") + rec(HS, hello(sni_ext(b"abc", host_len=0xFFF8))) + rec(APP, b"y"),
                                 [40])])
    add("empty_records_300", [conn(11, rec(APP) * 300, [700])])
    add("port_table", [conn(12, flight(b"alt.example"), [60], dport=8443) + conn(13, flight(b"web.example"), [60], dport=80)])
    add("quirks", [quirk_streams()])
    for n in (63, 64, 65, 255, 256, 257):
        add("streams_%d" % n, [[f for i in range(n) for f in conn(i, flight(b"s%d.example" % i), [33 + i % 200])]])
        add("records_%d" % n, [conn(14, rec(APP, b"ab") * n, [11])])
    # candidates only in the last block of 256 streams
    add("last_block", [[f for i in range(300) for f in conn(i, flight(b"l%d.example" % i), [70], dport=443 if i >= 290 else 80)]])
    return c


def random_mix(seed, nstreams, ncalls=3):
    """A seeded mix: per stream a random record list (now and then a record
    that fails, now and then bytes that are no TLS), random segment cuts,
    bounded reordering, a lost segment in about 5 % of the streams, a FIN in
    half of them; the streams' frames interleaved and dealt over `ncalls` calls."""
    rnd = random.Random(seed)
    per = []
    for i in range(nstreams):
        recs = []
        for _ in range(rnd.randrange(1, 6)):
            r = rnd.random()
            if r < 0.3:
                recs.append(hello_rec(b"r%d.example" % i, pad=rnd.randrange(0, 200)))
            elif r < 0.7:
                recs.append(rec(APP, bytes(rnd.randrange(0, 700))))
            elif r < 0.8:
                recs.append(rec(CCS, b"\x01"))
            elif r < 0.88:
                recs.append(rec(ALERT, bytes([rnd.randrange(1, 3), rnd.randrange(0, 60)])))
            elif r < 0.94:
                recs.append(rec(HS, hs_body(rnd.choice([2, 11, 16]), rnd.randrange(4, 80))))
            elif r < 0.97:
                recs.append(rec(CCS, b"\x01\x01"))
            else:
                recs.append(bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 30))))
        msg = b"".join(recs)
        if rnd.random() < 0.2:
            msg = msg[:rnd.randrange(1, len(msg) + 1)]
        cuts = sorted(set(rnd.randrange(1, max(2, len(msg))) for _ in range(rnd.randrange(0, 6))))
        nseg = len(cut(msg, cuts))
        order = list(range(nseg))
        for k in range(nseg - 1):
            if rnd.random() < 0.15:
                order[k], order[k + 1] = order[k + 1], order[k]
        drop = (rnd.randrange(nseg),) if rnd.random() < 0.05 and nseg > 1 else ()
        order = [k for k in range(nseg - len(drop))] if drop else order
        per.append(conn(i, msg, cuts, dport=rnd.choice([443, 443, 443, 993, 8443, 80]), syn=rnd.random() > 0.03,
                        fin=rnd.random() < 0.5, drop=drop, order=order))
    calls = [[] for _ in range(ncalls)]
    for fr in per:
        marks = sorted(rnd.randrange(0, len(fr) + 1) for _ in range(ncalls - 1))
        edges = [0] + marks + [len(fr)]
        for k in range(ncalls):
            calls[k].append(fr[edges[k]:edges[k + 1]])
    out = []
    for parts in calls:  # interleave the streams' frames inside a call
        mixed, idx = [], [0] * len(parts)
        live = [k for k in range(len(parts)) if parts[k]]
        while live:
            k = rnd.choice(live)
            mixed.append(parts[k][idx[k]])
            idx[k] += 1
            if idx[k] == len(parts[k]):
                live.remove(k)
        out.append(mixed)
    return out
