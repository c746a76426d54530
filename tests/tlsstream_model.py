"""Executable statement of TLS over reassembled streams
(include/gpk_tls_streams.h), independent of the C++ in
gopacket_amd/csrc/gpk_tls_streams.hip. TEST INFRASTRUCTURE ONLY.

It composes tcpasm_model.run (the reassembly) with tls_model.decode_message on
each record's own bytes: read 5 header bytes, read Length more, decode a buffer
of exactly that record. The terminal rules are stated here in plain Python.

  frame(buf, lost, closed)   one stream's logical buffer -> state, consumed, entries
  candidate(T, pkt, lay)     TCP.NextLayerType() of the creating packet is TLS
  asm_arrays(r)              a tcpasm_model.run result as gpk_tcp_streams arrays
  decode(...)                gpk_tls_streams' outputs for one call
  Streaming                  the model over several calls, state per global id
"""
import numpy as np

import pktutil
import tcpasm_model as AM
import tls_model as M
import tunnel_model as TM
from configs import oracle_parser
from gopacket_amd import _lib

NEW, SYNCED, NONE, NOSTART, NOT_TLS, LOST, CLOSED = range(7)
MAX_TAIL = 5 + 65535 - 1
NO_HELLO = 0xFFFFFFFF


def failed(err, off, hdr=None, a0=0, a1=0):
    ct, ver, ln = hdr if hdr else (0, 0, 0)
    return dict(content_type=ct, version=ver, length=ln, body_off=off + 5, err=err, err_a0=a0, err_a1=a1,
                status=1 if err in M.TRUNCATES else 0)


def frame(buf, lost, closed):
    """The obvious program over the stream's bytes. -> (state, consumed, entries);
    the tail is buf[consumed:] when the state is SYNCED."""
    off, out = 0, []
    while len(buf) - off >= 5:
        hdr = (buf[off], buf[off + 1] << 8 | buf[off + 2], buf[off + 3] << 8 | buf[off + 4])
        if not 20 <= hdr[0] <= 23:
            out.append(failed(M.E_REC_TYPE, off, hdr))
            return NOT_TLS, off + 5, out
        if len(buf) - off < 5 + hdr[2]:
            break
        rec = bytes(buf[off:off + 5 + hdr[2]])  # make([]byte, 5+Length)
        try:
            (r,) = M.decode_message(rec, 0, len(rec))
            r = dict(r, err=0, err_a0=0, err_a1=0, status=0)
            r["body_off"] += off
            if "client_hello" in r:
                h = r["client_hello"] = dict(r["client_hello"])
                for k in ("random_off", "session_id_off", "cipher_suits_off", "compression_methods_off",
                          "extensions_off"):
                    h[k] += off
                if h["has_sni"]:
                    h["sni_off"] += off
            out.append(r)
        except M.GoError as e:
            out.append(failed(e.code, off, hdr, e.a0, e.a1))
        off += 5 + hdr[2]
    rest = len(buf) - off
    if lost or closed:
        if rest:  # DecodeFromBytes(rest)
            h = (buf[off], buf[off + 1] << 8 | buf[off + 2], buf[off + 3] << 8 | buf[off + 4]) if rest >= 5 else None
            out.append(failed(M.E_LEN if rest >= 5 else M.E_REC_SHORT, off, h))
        return (LOST if lost else CLOSED), off, out
    return SYNCED, off, out


def candidate(T, pkt, lay):
    s, e = int(lay["start"][AM.SLOT_TCP]), int(lay["end"][AM.SLOT_TCP])
    return TM.last_payload(T, "TCP", pkt, s, e)[2] == M.LT_TLS


def asm_arrays(r, n):
    """A tcpasm_model.run result as the arrays of gpk_tcp_streams (n packets)."""
    S = len(r["streams"])
    chunks, data0, blob = [], [0], bytearray()
    for j, st in enumerate(r["streams"]):
        for ch in st["chunks"]:
            c = np.zeros(1, _lib.TCP_CHUNK_DTYPE)
            call = ch["call"]
            c["dst"], c["skip"], c["src"], c["src_off"], c["len"] = len(blob), ch["skip"], ch["src"], ch["src_off"], ch["len"]
            c["call"], c["stream"], c["flags"] = call, j, ch["flags"]
            chunks.append(c[0])
            blob += st["data"][len(blob) - data0[j]:len(blob) - data0[j] + ch["len"]]
        assert len(blob) - data0[j] == len(st["data"])
        data0.append(len(blob))
    pad = max(n - S, 0)
    return dict(chunks=np.array(chunks, _lib.TCP_CHUNK_DTYPE) if chunks else np.zeros(0, _lib.TCP_CHUNK_DTYPE),
                stream_first=np.array([st["first"] for st in r["streams"]] + [0] * pad, np.uint32),
                stream_closed=np.array([st["closed"] for st in r["streams"]] + [0] * pad, np.uint32),
                stream_data0=np.array(data0 + [0] * pad, np.uint64),
                counts=np.array([S, len(chunks), len(blob), 0, 0, 0, 0, 0], np.uint64),
                data=np.frombuffer(bytes(blob) + bytes(16), np.uint8), data_cap=len(blob), chunk_cap=len(chunks))


def stream_results(cfg, packets, layouts, r, carry=None, frame_unstarted=False):
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
        d["framed"], d["tail_in"] = True, len(tail)
        d["state"], d["consumed"], d["entries"] = frame(buf, lost, st["closed"] != AM.OPEN)
        if d["state"] == SYNCED:
            d["tail"] = buf[d["consumed"]:]
            assert len(d["tail"]) <= MAX_TAIL
    return res


def to_arrays(res, n, caps=(None,) * 4, fill=0):
    """gpk_tls_streams' outputs from stream_results, for a batch of n packets."""
    need = [sum(len(d["entries"]) for d in res), sum("client_hello" in e for d in res for e in d["entries"]),
            sum(e["client_hello"]["sni_len"] for d in res for e in d["entries"] if "client_hello" in e),
            sum(len(d["tail"]) for d in res)]
    caps = [x if c is None else c for x, c in zip(need, caps)]

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(streams=arr(max(n, 1), _lib.TLS_STREAM_DTYPE), recs=arr(caps[0], _lib.TLS_STREAM_REC_DTYPE),
               hellos=arr(caps[1], _lib.TLS_HELLO_DTYPE), snis=arr(caps[2], np.uint8), tails=arr(caps[3], np.uint8),
               counts=np.zeros(12, np.uint64))
    t = [0, 0, 0, 0]
    nframed = nfailed = 0
    for j, d in enumerate(res):
        rows, hrows, blob = [], [], bytearray()
        for e in d["entries"]:
            row = np.zeros(1, _lib.TLS_STREAM_REC_DTYPE)
            for name in ("content_type", "version", "length", "body_off", "hs", "v0", "v1"):
                if name in e:
                    row["rec"][name] = e[name]
            row["rec"]["hello"] = NO_HELLO
            for name in ("err", "err_a0", "err_a1", "status"):
                row[name] = e[name]
            row["stream"] = j
            if "client_hello" in e:
                h = e["client_hello"]
                row["rec"]["hello"] = len(hrows)
                hrow = np.zeros(1, _lib.TLS_HELLO_DTYPE)
                for name in _lib.TLS_HELLO_DTYPE.names:
                    if name in h:
                        hrow[name] = h[name]
                hrow["packet"], hrow["sni_pos"] = j, t[2] + len(blob)
                blob += h["sni"]
                hrows.append(hrow[0])
            rows.append(row[0])
        own = [len(rows), len(hrows), len(blob), len(d["tail"])]
        s = np.zeros(1, _lib.TLS_STREAM_DTYPE)
        s["state"], s["tail_in"], s["consumed"], s["tail_len"] = d["state"], d["tail_in"], d["consumed"], own[3]
        s["status"] = d.get("status", 0)
        s["nrec"], s["nfailed"] = own[0], sum(bool(e["err"]) for e in d["entries"])
        s["nhello"], s["sni_bytes"] = own[1], own[2]
        s["rec0"], s["hello0"], s["sni0"], s["tail_off"] = t[0], t[1], t[2], t[3]
        if d["framed"]:
            nframed += 1
            if all(a + b <= c for a, b, c in zip(t, own, caps)):
                for k, row in enumerate(rows):
                    out["recs"][t[0] + k] = row
                for k, row in enumerate(hrows):
                    out["hellos"][t[1] + k] = row
                out["snis"][t[2]:t[2] + own[2]] = np.frombuffer(bytes(blob), np.uint8)
                out["tails"][t[3]:t[3] + own[3]] = np.frombuffer(bytes(d["tail"]), np.uint8)
            else:
                s["status"] |= _lib.TLSS_ST_DROPPED
        nfailed += int(s["nfailed"][0])
        out["streams"][j] = s[0]
        t = [a + b for a, b in zip(t, own)]
    if res:
        out["counts"][:10] = [len(res), nframed, t[0], nfailed, t[1], int(any(a > c for a, c in zip(t, caps))),
                              t[0], t[1], t[2], t[3]]
    return out


def decode_call(cfg, packets, max_pages=0, flush=False, carry_asm=(), carry=None, frame_unstarted=False):
    """One call: oracle decode, reassembly model, stream results.
    -> (stream results, tcpasm result, (data, offsets, caplens, oracle results))"""
    data, off, cap = pktutil.pack(packets)
    ref = oracle_parser(cfg).decode(data, off, cap, layouts=True)
    r = AM.run(packets, ref["records"], ref["layouts"], max_pages=max_pages, flush=flush, carry=carry_asm)
    return stream_results(cfg, packets, ref["layouts"], r, carry, frame_unstarted), r, (data, off, cap, ref)


class Streaming:
    """The model over several calls, as flows.TLSStreams feeds the device: the
    open connections and their listed pages go in front of the next batch as
    carried entries; state and tail are kept per global stream id."""

    def __init__(self, cfg, max_pages=0, frame_unstarted=False):
        self.cfg, self.max_pages, self.frame_unstarted = cfg, max_pages, frame_unstarted
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
        res = stream_results(self.cfg, pk, ref["layouts"], r, carry, self.frame_unstarted)
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
