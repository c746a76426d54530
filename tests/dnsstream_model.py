"""Executable statement of DNS over reassembled streams
(include/gpk_dns_streams.h), independent of the C++ in
gopacket_amd/csrc/gpk_dns_streams.hip. TEST INFRASTRUCTURE ONLY.

It composes tcpasm_model.run (the reassembly) with dns_model.decode_message on
each message's own bytes: read 2 length bytes, read Length more, decode a buffer
of exactly that message. The framing, terminal, candidate, skip and capacity
rules are stated here in plain Python.

  frame(buf, lost, closed, cap)  one stream's logical buffer -> state, consumed, entries
  candidate(T, pkt, lay)         TCP.NextLayerType() of the creating packet is DNS
  decode(...)                    gpk_dns_streams' outputs for one call (to_arrays)
  Streaming                      the model over several calls, state per global id
"""
import sys

import numpy as np

import dns_model as M
import pktutil
import tcpasm_model as AM
import tunnel_model as TM
from configs import oracle_parser
from gopacket_amd import _lib
from tlsstream_model import asm_arrays  # noqa: F401  (the reassembly as gpk_tcp_streams arrays: no TLS in it)

NEW, SYNCED, NONE, NOSTART, LOST, CLOSED = range(6)
PARTIAL, SKIPPED, DROPPED = 1, 2, 4
MAX_TAIL = 2 + 65535 - 1


def frame(buf, lost, closed, cap=0):
    """The obvious program over the stream's bytes. -> (state, consumed, entries);
    the tail is buf[consumed:] when the state is SYNCED. An entry is
    dict(hdr_off, len, present, mstatus) and, when it was decoded, either
    "msg" (dns_model.decode_message's dict) or "err", "err_a0", "err_a1"."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
    cap = cap or 65535
    off, out = 0, []
    while len(buf) - off >= 2:
        ln = buf[off] << 8 | buf[off + 1]
        if len(buf) - off - 2 < ln:
            break
        e = dict(hdr_off=off + 2, len=ln, present=2 + ln, mstatus=0)
        if ln > cap:
            e["mstatus"] = SKIPPED
        else:
            msg = bytes(buf[off + 2:off + 2 + ln])  # make([]byte, Length)
            try:
                e["msg"] = M.decode_message(msg, off + 2)
            except M.GoError as x:
                e.update(err=x.code, err_a0=x.a0, err_a1=x.a1)
        out.append(e)
        off += 2 + ln
    rest = len(buf) - off
    if lost or closed:
        if rest:  # io.ReadFull fails
            out.append(dict(hdr_off=off + 2, len=(buf[off] << 8 | buf[off + 1]) if rest >= 2 else 0, present=rest,
                            mstatus=PARTIAL))
        return (LOST if lost else CLOSED), off, out
    return SYNCED, off, out


def candidate(T, pkt, lay):
    s, e = int(lay["start"][AM.SLOT_TCP]), int(lay["end"][AM.SLOT_TCP])
    return TM.last_payload(T, "TCP", pkt, s, e)[2] == M.LT_DNS


def stream_results(cfg, packets, layouts, r, carry=None, frame_unstarted=False, max_message=0):
    """Per stream of a tcpasm_model.run result: dict(state, framed, tail_in,
    consumed, entries, tail). carry: per stream (state, tail bytes) or None."""
    T = TM.Tables(cfg)
    res = []
    for j, st in enumerate(r["streams"]):
        state, tail = carry[j] if carry and j < len(carry) and carry[j] else (NEW, b"")
        d = dict(state=state, framed=False, tail_in=0, consumed=0, entries=[], tail=b"")
        res.append(d)
        if state not in (NEW, SYNCED):
            continue
        if state == NEW and not candidate(T, packets[st["first"]], layouts[st["first"]]):
            d["state"] = NONE
            continue
        if any(ch["skip"] < 0 for ch in st["chunks"]) and not frame_unstarted:
            d["state"] = NOSTART
            continue
        tail = tail if state == SYNCED else b""
        new, at, lost = st["data"], 0, False
        for ch in st["chunks"]:  # cut at the first chunk with Skip > 0
            if ch["skip"] > 0:
                new, lost = new[:at], True
                break
            at += ch["len"]
        buf = bytes(tail) + bytes(new)
        d["framed"], d["tail_in"], d["buf"] = True, len(tail), buf
        d["state"], d["consumed"], d["entries"] = frame(buf, lost, st["closed"] != AM.OPEN, max_message)
        if d["state"] == SYNCED:
            d["tail"] = buf[d["consumed"]:]
            assert len(d["tail"]) <= MAX_TAIL
    return res


def rr_rows(m, name0):
    """(gpk_dns_rr rows, name bytes) of a decoded message whose names start at name0 of the arena."""
    rows, blob = [], bytearray()
    for r in m["rrs"]:
        row = np.zeros(1, _lib.DNS_RR_DTYPE)
        for name in ("section", "type", "cls", "data_length", "ttl", "data_off", "count", "v"):
            if name in r:
                row[name] = r[name]
        for key, o_, l_ in (("name", "name_off", "name_len"), ("rname", "rname_off", "rname_len"),
                            ("rname2", "rname2_off", "rname2_len")):
            if key in r:
                row[o_], row[l_] = name0 + len(blob), len(r[key])
                blob += r[key]
        rows.append(row[0])
    return rows, bytes(blob)


def to_arrays(res, n, caps=(None,) * 4, fill=0):
    """gpk_dns_streams' outputs from stream_results, for a batch of n packets.
    caps: (msg, rr, name, tail); None: exactly what everything needs."""
    every = [e for d in res for e in d["entries"]]
    sized = [rr_rows(e["msg"], 0) if "msg" in e else ([], b"") for e in every]
    need = [len(every), sum(len(r) for r, _ in sized), sum(len(b) for _, b in sized), sum(len(d["tail"]) for d in res)]
    caps = [x if c is None else c for x, c in zip(need, caps)]

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(streams=arr(max(n, 1), _lib.DNS_STREAM_DTYPE), msgs=arr(caps[0], _lib.DNS_STREAM_MSG_DTYPE),
               rrs=arr(caps[1], _lib.DNS_RR_DTYPE), names=arr(caps[2], np.uint8), tails=arr(caps[3], np.uint8),
               counts=np.zeros(12, np.uint64))
    tm = tt = rr0 = name0 = 0
    nframed = nfailed = 0
    over = False
    for j, d in enumerate(res):
        own_m, own_t = len(d["entries"]), len(d["tail"])
        s = np.zeros(1, _lib.DNS_STREAM_DTYPE)
        s["state"], s["tail_in"], s["consumed"], s["tail_len"] = d["state"], d["tail_in"], d["consumed"], own_t
        s["status"] = d.get("status", 0)
        s["nmsg"], s["msg0"], s["tail_off"] = own_m, tm, tt
        if d["framed"]:
            nframed += 1
            if tm + own_m <= caps[0] and tt + own_t <= caps[3]:  # level one: the stream, whole or not at all
                out["tails"][tt:tt + own_t] = np.frombuffer(bytes(d["tail"]), np.uint8)
                for k, e in enumerate(d["entries"]):
                    row = np.zeros(1, _lib.DNS_STREAM_MSG_DTYPE)
                    row["stream"], row["status"], row["present"] = j, e["mstatus"], e["present"]
                    t = row["msg"]
                    t["kind"], t["hdr_off"] = 1, e["hdr_off"]
                    if e["mstatus"]:
                        t["len"] = e["len"]
                    elif "err" in e:
                        t["err"], t["err_a0"], t["err_a1"] = e["err"], e["err_a0"], e["err_a1"]
                        t["status"] = 1 if e["err"] == M.E_SHORT else 0
                        s["nfailed"] += 1
                    else:
                        m = e["msg"]
                        for name in _lib.DNS_DTYPE.names:
                            if name in m:
                                t[name] = m[name]
                        rows, blob = rr_rows(m, name0)
                        t["nrr"], t["name_bytes"], t["rr0"], t["name0"] = len(rows), len(blob), rr0, name0
                        if rr0 + len(rows) <= caps[1] and name0 + len(blob) <= caps[2]:  # level two: the message
                            for i, rw in enumerate(rows):
                                out["rrs"][rr0 + i] = rw
                            out["names"][name0:name0 + len(blob)] = np.frombuffer(blob, np.uint8)
                        else:
                            row["status"] |= DROPPED
                            over = True
                        rr0 += len(rows)
                        name0 += len(blob)
                    row["msg"] = t
                    out["msgs"][tm + k] = row[0]
            else:
                s["status"] |= _lib.DNSS_ST_DROPPED
                over = True
        nfailed += int(s["nfailed"][0])
        out["streams"][j] = s[0]
        tm += own_m
        tt += own_t
    if res:
        out["counts"][:9] = [len(res), nframed, tm, nfailed, int(over), tm, rr0, name0, tt]
    return out


class Streaming:
    """The model over several calls, as flows.DNSStreams feeds the device: the
    open connections and their listed pages go in front of the next batch as
    carried entries; state and tail are kept per global stream id."""

    def __init__(self, cfg, max_pages=0, frame_unstarted=False, max_message=0):
        self.cfg, self.max_pages, self.frame_unstarted, self.max_message = cfg, max_pages, frame_unstarted, max_message
        self.carried = []  # (packet, code, seq, global id)
        self.state = {}    # global id -> (state, tail)
        self.ids = 0
        self.last = None

    def feed(self, packets, flush=False):
        """-> [dict(id, state, framed, tail_in, consumed, entries, tail, closed)] in stream order"""
        P = len(self.carried)
        pk = [c[0] for c in self.carried] + list(packets)
        if not pk:
            self.last = None
            return []
        data, off, cap = pktutil.pack(pk)
        ref = oracle_parser(self.cfg).decode(data, off, cap, layouts=True)
        r = AM.run(pk, ref["records"], ref["layouts"], max_pages=self.max_pages, flush=flush,
                   carry=[(c[1], c[2]) for c in self.carried])
        ids = []
        for st in r["streams"]:
            if st["first"] >= P:
                ids.append(self.ids)
                self.ids += 1
            else:
                ids.append(self.carried[st["first"]][3])
        carry = [self.state.get(g) for g in ids]
        res = stream_results(self.cfg, pk, ref["layouts"], r, carry, self.frame_unstarted, self.max_message)
        self.last = dict(packets=pk, arrays=(data, off, cap, ref), asm=r, carry=carry, res=res, ids=ids)
        for g, d, st in zip(ids, res, r["streams"]):
            d["id"], d["closed"] = g, st["closed"] != AM.OPEN
            if d["closed"]:
                self.state.pop(g, None)
            else:
                self.state[g] = (d["state"], d["tail"])
        nxt = []
        pages = {}
        for p, k in r["pend"]:
            pages.setdefault(r["streams"][r["stream_of"][p]]["group"], []).append((p, k))
        for g in range(r["groups"]):
            if r["conn_seq"][g] == AM.NO_CONN:
                continue
            s = r["conn_stream"][g]
            nxt.append((pk[r["streams"][s]["first"]], AM.CARRY_CONN, r["conn_seq"][g], ids[s]))
            nxt += [(pk[p], AM.CARRY_PAGE | k, 0, ids[s]) for p, k in pages.get(g, ())]
        self.carried = nxt
        return res

    def flush_all(self):
        return self.feed([], flush=True)


def decoded(res):
    """[(global id, message dict)] of the messages of a call result that decoded."""
    return [(d["id"], e["msg"]) for d in res for e in d["entries"] if "msg" in e]


def questions(res):
    """[(global id, name, type)] as DNSStreamResult.questions()."""
    return [(g, r["name"], r["type"]) for g, m in decoded(res) for r in m["rrs"] if r["section"] == 0]
