"""Packets for the DNS-over-streams tests (include/gpk_dns_streams.h): TCP
connections that carry length-prefixed DNS messages cut into segments, built
with tlsstreamcases.conn and the message builders of dnscases.

A case is dict(name, calls=[[packet, ...], ...], max_pages, frame_unstarted,
max_message, flush, parser): the calls are fed in order and, with flush, a
FlushAll follows.
"""
import random
import struct

import dnscases as C
import tcpasmcases as TC
from dnscases import A, AAAA, CNAME, MX, OPT, TXT, hdr, name, q, rr
from tlsstreamcases import addr, conn, cut

PARSER = C.PARSER                                      # 53 by default, 8080 registered
PARSER_5353 = dict(C.PARSER, tcp_port={5353: 107, 53: 2})  # 5353 registered, 53 unregistered (LayerTypePayload)
SYN, FIN = TC.SYN, TC.FIN
MSS = 1448
QUIRK_MAX = 300  # no long pointer chain: a quadratic walk must not occupy a shared device


def pre(msg):
    """The message behind its two length bytes (RFC 1035 4.2.2)."""
    return struct.pack(">H", len(msg)) + msg


def query(ident=0x1234):
    """A 29-byte query for example.com A."""
    m = hdr(1, flags=0x0100, ident=ident) + C.QEX
    assert len(m) == 29
    return m


def response(ident=0x1234):
    """Six entries behind the question: A, AAAA, a CNAME whose target ends in a
    pointer, MX, TXT and an OPT in the additional section."""
    return (hdr(1, 5, 0, 1, ident=ident) + C.QEX + rr(C.P, A, bytes([192, 0, 2, 1])) + rr(C.P, AAAA, bytes(range(16))) +
            rr(C.P, CNAME, name(b"www", ptr=12)) + rr(C.P, MX, struct.pack(">H", 10) + name(b"mail", ptr=12)) +
            rr(C.P, TXT, b"\x03abc\x05hello") +
            rr(C.OPT0, OPT, struct.pack(">HH", 10, 8) + bytes(8), cls=4096, ttl=0))


def exchange(ident=0x1234):
    """What the tests call "that stream": the query and the response, prefixed."""
    return pre(query(ident)) + pre(response(ident))


def small(i):
    """A small message: one question with a label that tells the messages apart."""
    return hdr(1, ident=i & 0xFFFF) + q(name(b"m%d" % i, b"zone", b"test"))


def zone(n, first=0):
    """n small prefixed messages: the zone-transfer shape."""
    return b"".join(pre(small(first + i)) for i in range(n))


def split_streams(two_calls):
    """One stream per byte position of exchange(): the payload in two segments
    cut there; k == 1 leaves half a prefix, k == 2 a prefix and no body. -> calls"""
    msg = exchange()
    a, b = [], []
    for k in range(1, len(msg)):
        fr = conn(k, msg, [k], dport=53)
        a += fr[:2]
        (b if two_calls else a).append(fr[2])
    return [a, b] if two_calls else [a]


def seam_pointers():
    """Two streams in two calls. In the first the cut lies behind the question
    name, so the answers' pointers (in the new bytes) reach into the carried
    tail; in the second it lies inside "example", so their target straddles the
    seam."""
    msg = pre(response())
    behind, inside = 2 + 12 + 13 + 4, 2 + 12 + 4
    a, b = [], []
    for i, k in ((1, behind), (2, inside)):
        fr = conn(i, msg, [k], dport=53)
        a += fr[:2]
        b.append(fr[2])
    return [a, b]


def largest():
    """One message of Length 65535: a header, one question and one TXT record
    that fills the rest, over 46 segments and three calls, then a small one."""
    head = hdr(1, 1) + C.QEX + C.P + struct.pack(">HHIH", TXT, 1, 300, 65535 - 29 - 12)
    body = b""
    left = 65535 - len(head)
    while left:  # character-strings of at most 255 bytes
        n = min(255, left - 1)
        body += bytes([n]) + bytes((7 * k) & 255 for k in range(n))
        left -= 1 + n
    msg = pre(head + body) + pre(query(7))
    assert len(head + body) == 65535
    # the second call ends one byte short of the message: the tail peaks at 65536 bytes
    fr = conn(1, msg, [MSS * k for k in range(1, 45)] + [65536], dport=53)
    assert len(fr) == 1 + 46
    return [fr[:21], fr[21:46], fr[46:]]


def quirk_streams():
    """Every hand-built message of dnscases (the reference's error paths) as
    the one message of its own connection, closed by a FIN."""
    out = []
    for i, (nm, pkt) in enumerate(C.quirk_cases()[0]):
        if pkt[12:14] != b"\x08\x00" or pkt[23] != 17 or not 42 < len(pkt) <= 42 + QUIRK_MAX:
            continue
        out += conn(i, pre(pkt[42:]), [5], dport=53, fin=True)
    return out


def cases():
    c = []

    def add(name_, calls, max_pages=0, frame_unstarted=False, flush=False, max_message=0, parser=PARSER):
        c.append(dict(name=name_, calls=calls, max_pages=max_pages, frame_unstarted=frame_unstarted, flush=flush,
                      max_message=max_message, parser=parser))
    add("exchange", [conn(1, exchange(), [40], dport=53)])
    add("split_one_call", split_streams(False))
    add("split_two_calls", split_streams(True))
    add("seam_pointers", seam_pointers())
    add("largest_message", largest())
    add("length_0_and_11", [conn(1, pre(b"") + pre(bytes(11)) + pre(query()), [3], dport=53)])
    lim = len(response())
    add("max_message", [conn(1, pre(response()) + pre(response() + b"\x00") + pre(query()), [50], dport=53)],
        max_message=lim)
    many = exchange() + zone(8)
    add("loss_in_front", [conn(1, many, [10, 31, 60], drop=(0,), dport=53)], flush=True)
    add("loss_inside", [conn(2, many, [10, 40, 60], drop=(1,), dport=53)], flush=True)
    add("loss_behind", [conn(3, many, [len(exchange()), len(exchange()) + 20], drop=(1,), dport=53)], flush=True)
    # the page limit pops a page behind a hole: LOST without a close; the second call carries the final state
    add("page_limit_forces_a_skip", [conn(4, exchange() + zone(20), [100, 300, 400, 500, 600], drop=(2,), dport=53),
                                     [TC.seg(1001 + len(exchange() + zone(20)), 0, pre(query(9)), src=addr(4)[0],
                                             sport=addr(4)[1], dport=53)]], max_pages=3)
    add("close_whole", [conn(5, exchange(), [40], dport=53, fin=True)])
    add("close_partial", [conn(6, exchange() + pre(response())[:60], [40], dport=53, fin=True) +
                          conn(7, exchange() + b"\x00", [40], dport=53, fin=True) +
                          conn(8, exchange() + b"\x00\x1d", [40], dport=53, fin=True)])
    add("loss_and_close", [conn(9, many, [10, 40, 60], drop=(1,), dport=53, fin=True)], flush=True)
    add("no_syn", [conn(10, exchange(), [40], dport=53, syn=False)], flush=True)
    add("no_syn_framed", [conn(10, exchange(), [40], dport=53, syn=False)], frame_unstarted=True, flush=True)
    add("server_direction", [conn(11, exchange(), [40], dport=50000, sport=53)])
    add("port_table", [conn(12, exchange(), [40], dport=5353) + conn(13, exchange(), [40], dport=53)], parser=PARSER_5353)
    add("port_8080_and_80", [conn(12, exchange(), [40], dport=8080) + conn(13, exchange(), [40], dport=80)])
    add("quirks", [quirk_streams()])
    for n in (63, 64, 65, 255, 256, 257):
        add("streams_%d" % n, [[f for i in range(n) for f in conn(i, exchange(i), [33 + i % 60], dport=53)]])
    for n in (63, 64, 65, 257):  # the entry range crosses streams: one in front, one behind
        add("messages_%d" % n, [conn(1, exchange(), [9], dport=53) + conn(2, zone(n), [11, 700], dport=53) +
                                conn(3, exchange(), [70], dport=53)])
    # candidates only in the last block of 256 streams
    add("last_block", [[f for i in range(300) for f in conn(i, exchange(i), [70], dport=53 if i >= 290 else 80)]])
    return c


def random_mix(seed, nstreams, ncalls=3):
    """A seeded mix: per stream a random message list (queries, responses,
    small messages, now and then a message that fails or a short one), random
    segment cuts, bounded reordering, a lost segment in about 5 % of the
    streams, a FIN in half of them, no SYN in about 3 %, other ports in a
    sixth; the streams' frames interleaved and dealt over `ncalls` calls."""
    rnd = random.Random(seed)
    quirks = [pkt[42:] for _, pkt in C.quirk_cases()[0] if pkt[12:14] == b"\x08\x00" and pkt[23] == 17 and 42 < len(pkt) <= 42 + QUIRK_MAX]
    per = []
    for i in range(nstreams):
        msgs = []
        for _ in range(rnd.randrange(1, 6)):
            r = rnd.random()
            if r < 0.3:
                msgs.append(pre(query(rnd.randrange(65536))))
            elif r < 0.6:
                msgs.append(pre(response(rnd.randrange(65536))))
            elif r < 0.8:
                msgs.append(pre(small(rnd.randrange(100000))))
            elif r < 0.92:
                msgs.append(pre(rnd.choice(quirks)))
            elif r < 0.96:
                msgs.append(pre(bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 12)))))
            else:
                m = bytearray(response())
                m[rnd.randrange(len(m))] ^= 1 << rnd.randrange(8)
                msgs.append(pre(bytes(m)))
        msg = b"".join(msgs)
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
        per.append(conn(i, msg, cuts, dport=rnd.choice([53, 53, 53, 53, 8080, 80]), syn=rnd.random() > 0.03,
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
