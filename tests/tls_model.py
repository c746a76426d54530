"""Executable statement of the TLS rules (include/gpk_tls.h),
independent of the C++ in gopacket_amd/csrc/gpk_tls_rules.h: layers/tls.go,
tls_handshake.go, tls_alert.go, tls_cipherspec.go and tls_appdata.go restated on
Go-style slices (a window of a buffer with a capacity), recursion and all.

  Slice                 a Go []byte: buffer, low, high, capacity end; slicing
                        checks its bounds the way the Go runtime does and
                        raises GoPanic with the runtime's text
  decode_records        TLS.decodeTLSRecords, tls.go:130-194 (recursive, as written)
  decode_ccs / decode_alert / decode_appdata / decode_handshake
                        the four decodeFromBytes
  is_encrypted          isEncryptedHandshakeMessage, tls_handshake.go:198-223
  decode_client_hello   tls_handshake.go:104-189, with the re-slice to the
                        capacity and the uint16 sums of the SNI reads
  tls_packet            the candidate rule, then decode_records
  tls(cfg, ...)         gpk_tls_batch's outputs
  compose(cfg, packets) DecodeLayers with layers.TLS (and, optionally, DNS, the
                        control and tunnel layers) added to the parser of `cfg`

A packet is a buffer of exactly its captured bytes (pcapgo.ReadPacketData):
the capacity of every slice ends at the packet's end. The candidate's payload
and next type come from tunnel_model.last_payload, and the six-layer decode of
every level is the oracle's (oracle/).
"""
import sys

import numpy as np

import tunnel_model as TM
from tunnel_model import Tables
from gopacket_amd import _lib

LT_TLS = 140
(E_REC_SHORT, E_REC_TYPE, E_LEN, E_CCS, E_ALERT, E_HS_SHORT, E_HS_TYPE, E_CH_SHORT, E_CH_SESSION, E_CH_CIPHERS,
 E_CH_COMPRESSION, E_CH_EXTENSIONS) = range(121, 133)
E_PANIC_SLICE_B = 4
ALL_ERRORS = tuple(range(121, 133)) + (E_PANIC_SLICE_B,)
TEXT = {
    E_REC_SHORT: "TLS record too short", E_REC_TYPE: "Unknown TLS record type", E_LEN: "TLS packet length mismatch",
    E_CCS: "TLS Change Cipher Spec record incorrect length", E_ALERT: "TLS Alert packet too short",
    E_HS_SHORT: "TLS handshake record too short", E_HS_TYPE: "Unknown TLS handshake type",
    E_CH_SHORT: "TLS ClientHello too short", E_CH_SESSION: "TLS ClientHello truncated in session ID",
    E_CH_CIPHERS: "TLS ClientHello truncated in cipher suites",
    E_CH_COMPRESSION: "TLS ClientHello truncated in compression methods",
    E_CH_EXTENSIONS: "TLS ClientHello truncated in extensions",
    E_PANIC_SLICE_B: "panic: runtime error: slice bounds out of range [%d:%d]"}
TRUNCATES = {E_REC_SHORT, E_LEN, E_CCS, E_ALERT, E_HS_SHORT, E_CH_SHORT, E_CH_SESSION, E_CH_CIPHERS, E_CH_COMPRESSION,
             E_CH_EXTENSIONS}
HANDSHAKE_TYPES = {0, 1, 2, 3, 11, 12, 13, 14, 15, 16, 20}  # handShakeTypeMap


class GoError(Exception):
    def __init__(self, code, a0=0, a1=0):
        Exception.__init__(self, code, a0, a1)
        self.code, self.a0, self.a1 = code, a0, a1


def error_text(code, a0=0, a1=0):
    if code == 0:
        return ""
    t = TEXT[code]
    return t % (a0, a1) if "%" in t else t


class Slice:
    """A Go byte slice: buf[lo:hi] with capacity to `end`."""

    def __init__(self, buf, lo=0, hi=None, end=None):
        self.buf, self.lo = buf, lo
        self.hi = len(buf) if hi is None else hi
        self.end = len(buf) if end is None else end

    def __len__(self):
        return self.hi - self.lo

    def cap(self):
        return self.end - self.lo

    def __getitem__(self, i):
        if isinstance(i, slice):
            lo = 0 if i.start is None else i.start
            hi = len(self) if i.stop is None else i.stop
            if hi > self.cap():
                raise AssertionError("slice bounds out of range [:%d] with capacity %d: not on the TLS path" %
                                     (hi, self.cap()))
            if lo > hi:
                raise GoError(E_PANIC_SLICE_B, lo, hi)
            return Slice(self.buf, self.lo + lo, self.lo + hi, self.end)
        assert 0 <= i < len(self), "index out of range [%d] with length %d: not on the TLS path" % (i, len(self))
        return self.buf[self.lo + i]

    def bytes(self):
        return bytes(self.buf[self.lo:self.hi])


def be16(d, i=0):
    return d[i] << 8 | d[i + 1]


def u16(x):
    return x & 0xFFFF


def u32(x):
    return x & 0xFFFFFFFF


def header(h):
    return dict(content_type=h[0], version=h[1], length=h[2])


def decode_ccs(h, data):
    if len(data) != 1:
        raise GoError(E_CCS)
    return dict(header(h), v0=1 if data[0] == 1 else 255)


def decode_alert(h, data):
    if len(data) < 2:
        raise GoError(E_ALERT)
    if h[2] == 2:
        return dict(header(h), v0=data[0], v1=data[1])
    return dict(header(h), v0=255, v1=255, encrypted=data.bytes())


def decode_appdata(h, data):
    assert len(data) == h[2]  # "TLS Application Data length mismatch" cannot occur
    return dict(header(h), payload=data.bytes())


def is_encrypted(h, data):
    if h[2] < 16:
        return False
    maybe_type = data[0]
    d = [0, 0, 0, 0]
    for k, v in enumerate(data[1:4].bytes()):
        d[k + 1] = v
    if u32(h[2] - (d[0] << 24 | d[1] << 16 | d[2] << 8 | d[3])) != 4:
        return True
    return maybe_type not in HANDSHAKE_TYPES


def decode_client_hello(data):
    """tls_handshake.go:104-189; the offsets in the result are absolute in the buffer."""
    data = data[:data.cap()]
    if len(data) < 39:
        raise GoError(E_CH_SHORT)
    t = dict(handshake_type=data[0], length=data[1] << 16 | data[2] << 8 | data[3], protocol_version=be16(data, 4),
             random_off=data.lo + 6, session_id_length=data[38], has_sni=0, sni_off=0, sni_len=0, sni=b"")
    pos = 39 + t["session_id_length"]
    if len(data) < pos + 2:
        raise GoError(E_CH_SESSION)
    t["session_id_off"] = data.lo + 39
    t["cipher_suits_length"] = be16(data[pos:pos + 2])
    pos += 2
    if len(data) < pos + t["cipher_suits_length"] + 1:
        raise GoError(E_CH_CIPHERS)
    t["cipher_suits_off"] = data.lo + pos
    pos += t["cipher_suits_length"]
    t["compression_methods_length"] = data[pos]
    pos += 1
    if len(data) < pos + t["compression_methods_length"] + 2:
        raise GoError(E_CH_COMPRESSION)
    t["compression_methods_off"] = data.lo + pos
    pos += t["compression_methods_length"]
    t["extensions_length"] = be16(data[pos:pos + 2])
    pos += 2
    if len(data) < pos + t["extensions_length"]:
        raise GoError(E_CH_EXTENSIONS)
    data = data[pos:pos + t["extensions_length"]]
    t["extensions_off"] = data.lo
    while len(data) > 0:
        if len(data) < 4:
            break
        extension_type = be16(data[:2])
        length = be16(data[2:4])
        if len(data) < 4 + length:
            break
        if extension_type == 0:
            if len(data) > 6:
                server_name_extension_length = be16(data[4:6])
                entry_type = data[6]
                if server_name_extension_length > 0 and entry_type == 0 and len(data) > 8:
                    hostname_length = be16(data[7:9])
                    if len(data) > u16(8 + hostname_length):
                        sni = data[9:u16(9 + hostname_length)]
                        t["has_sni"], t["sni_off"], t["sni_len"], t["sni"] = 1, sni.lo, len(sni), sni.bytes()
        data = data[u16(4 + length):]
    return t


def decode_handshake(h, data):
    r = dict(header(h), hs=_lib.TLS_HS_NONE)
    if is_encrypted(h, data):
        return dict(r, hs=_lib.TLS_HS_ENCRYPTED)
    if len(data) < 1:
        raise GoError(E_HS_SHORT)
    if data[0] == 1:
        return dict(r, hs=_lib.TLS_HS_CLIENT_HELLO, client_hello=decode_client_hello(data))
    if data[0] == 16:
        return dict(r, hs=_lib.TLS_HS_CLIENT_KEY)
    raise GoError(E_HS_TYPE)


def decode_records(data, out):
    """tls.go:130-194; appends one dict per record to out (body_off absolute in the buffer)."""
    if len(data) < 5:
        raise GoError(E_REC_SHORT)
    h = (data[0], be16(data[1:3]), be16(data[3:5]))
    if not 20 <= h[0] <= 23:
        raise GoError(E_REC_TYPE)
    hl = 5
    tl = hl + h[2]
    if len(data) < tl:
        raise GoError(E_LEN)
    body = data[hl:tl]
    r = {20: decode_ccs, 21: decode_alert, 22: decode_handshake, 23: decode_appdata}[h[0]](h, body)
    r["body_off"] = body.lo
    out.append(r)
    if len(data) == tl:
        return
    decode_records(data[tl:len(data)], out)


def decode_message(pkt, off, ln):
    """TLS.DecodeFromBytes(pkt[off:off+ln]) with the packet as the buffer: the record list; raises GoError."""
    out = []
    decode_records(Slice(pkt, off, off + ln), out)
    return out


def tls_packet(T, pkt, rec, lay, err_a0):
    """One packet: (class or TLS_NONE / TLS_UNKNOWN, message dict or None)."""
    status = int(rec["status"])
    nl = (status >> 8) & 0xfff
    if nl > 16:
        return _lib.TLS_UNKNOWN, None
    err = status & 0x7f
    if nl == 0 or err not in (0, 1):
        return _lib.TLS_NONE, None
    dec = TM.CODE_DEC[(int(rec["layers"]) >> (4 * (nl - 1))) & 15]
    if dec in ("PAYLOAD", "FRAGMENT"):
        return _lib.TLS_NONE, None
    k = TM.SLOTS.index(dec)
    off, ln, nxt = TM.last_payload(T, dec, pkt, int(lay["start"][k]), int(lay["end"][k]))
    if err == 1 and err_a0 is not None:
        assert nxt == err_a0, (nxt, err_a0)
    if nxt != LT_TLS or ln == 0:
        return _lib.TLS_NONE, None
    try:
        recs = decode_message(pkt, off, ln)
    except GoError as e:
        return _lib.TLS_CLASS_FAILED, dict(err=e.code, err_a0=e.a0, err_a1=e.a1, hdr_off=off,
                                           status=1 if e.code in TRUNCATES else 0, recs=[])
    return _lib.TLS_CLASS_OK, dict(hdr_off=off, len=ln, recs=recs)


def tls(cfg, data, offsets, caplens, records, layouts, err_args=None, rec_cap=None, hello_cap=None, sni_cap=None,
        fill=0):
    """gpk_tls_batch's outputs (arrays start as `fill` bytes). A capacity of
    None: exactly what the batch needs."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    T = Tables(cfg)
    n = len(caplens)
    raw = bytes(np.ascontiguousarray(data, np.uint8))
    res = []
    for i in range(n):
        o, c = int(offsets[i]), int(caplens[i])
        a0 = int(err_args[2 * i]) if err_args is not None else None
        if a0 is not None and a0 >= 1 << 31:
            a0 -= 1 << 32
        res.append(tls_packet(T, raw[o:o + c], records[i], layouts[i], a0))
    hellos_of = lambda m: [r["client_hello"] for r in m["recs"] if "client_hello" in r]  # noqa: E731
    need_rec = sum(len(m["recs"]) for c, m in res if c == 0)
    need_hello = sum(len(hellos_of(m)) for c, m in res if c == 0)
    need_sni = sum(h["sni_len"] for c, m in res if c == 0 for h in hellos_of(m))
    rec_cap = need_rec if rec_cap is None else rec_cap
    hello_cap = need_hello if hello_cap is None else hello_cap
    sni_cap = need_sni if sni_cap is None else sni_cap

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(verdict=arr(n, np.int32), class_start=arr(3, np.uint32), index=arr(n, np.uint32),
               records=arr(n, _lib.TLS_DTYPE), counts=arr(12, np.uint32), recs=arr(rec_cap, _lib.TLS_REC_DTYPE),
               hellos=arr(hello_cap, _lib.TLS_HELLO_DTYPE), snis=arr(sni_cap, np.uint8))
    j = rec0 = hello0 = sni0 = 0
    for c in range(_lib.TLS_NCLASS):
        out["class_start"][c] = j
        for i, (cls, m) in enumerate(res):
            if cls != c:
                continue
            out["verdict"][i] = j
            out["index"][j] = i
            rec = np.zeros(1, _lib.TLS_DTYPE)
            for name in ("err", "err_a0", "err_a1", "status", "hdr_off", "len"):
                if name in m:
                    rec[name] = m[name]
            if c == 0:
                rows, hrows, blob = [], [], bytearray()
                for r in m["recs"]:
                    row = np.zeros(1, _lib.TLS_REC_DTYPE)
                    for name in ("content_type", "version", "length", "body_off", "hs", "v0", "v1"):
                        if name in r:
                            row[name] = r[name]
                    row["hello"] = _lib.TLS_NO_HELLO
                    if "client_hello" in r:
                        h = r["client_hello"]
                        row["hello"] = len(hrows)
                        hrow = np.zeros(1, _lib.TLS_HELLO_DTYPE)
                        for name in _lib.TLS_HELLO_DTYPE.names:
                            if name in h:
                                hrow[name] = h[name]
                        hrow["packet"], hrow["sni_pos"] = i, sni0 + len(blob)
                        blob += h["sni"]
                        hrows.append(hrow[0])
                    rows.append(row[0])
                rec["nrec"], rec["nhello"], rec["sni_bytes"] = len(rows), len(hrows), len(blob)
                for key, ct in (("nccs", 20), ("nalert", 21), ("nhandshake", 22), ("nappdata", 23)):
                    rec[key] = sum(r["content_type"] == ct for r in m["recs"])
                rec["rec0"], rec["hello0"], rec["sni0"] = rec0, hello0, sni0
                if rec0 + len(rows) <= rec_cap and hello0 + len(hrows) <= hello_cap and sni0 + len(blob) <= sni_cap:
                    for k, row in enumerate(rows):
                        out["recs"][rec0 + k] = row
                    for k, row in enumerate(hrows):
                        out["hellos"][hello0 + k] = row
                    out["snis"][sni0:sni0 + len(blob)] = np.frombuffer(bytes(blob), np.uint8)
                else:
                    rec["status"] |= _lib.TLS_ST_DROPPED
                rec0 += len(rows)
                hello0 += len(hrows)
                sni0 += len(blob)
            out["records"][j] = rec[0]
            j += 1
    out["class_start"][2] = j
    for i, (cls, m) in enumerate(res):
        if cls < 0:
            out["verdict"][i] = cls
    out["counts"][:] = 0
    out["counts"][0] = j
    out["counts"][1:3] = np.diff(out["class_start"].astype(np.int64))
    if j:
        out["counts"][3] = int(need_rec > rec_cap or need_hello > hello_cap or need_sni > sni_cap)
        for k, need in ((4, need_rec), (6, need_hello), (8, need_sni)):
            out["counts"][k], out["counts"][k + 1] = need & 0xffffffff, need >> 32
    assert (rec0, hello0, sni0) == (need_rec, need_hello, need_sni)
    return out


def snis(out):
    """[(packet index, server name)] of tls() / TLSDecoder outputs, in packet order."""
    res = [(int(h["packet"]), bytes(out["snis"][int(h["sni_pos"]):int(h["sni_pos"]) + int(h["sni_len"])]))
           for h in out["hellos"] if int(h["has_sni"])]
    return sorted(res, key=lambda x: x[0])


def compose(cfg, packets, tls_on=True, dns_on=False, control_kinds=0, tunnel_kinds=0):
    """DecodeLayers of every packet with layers.TLS (and layers.DNS, the control
    layers `control_kinds`, the tunnel layers `tunnel_kinds`) added to the
    parser of `cfg`: dns_model's composition, then the TLS pass over every
    level's part. A TLS candidate's last layer leads to LayerTypeTLS, so it is
    no tunnel, control or DNS candidate. Every level entry gains "tls"."""
    import dns_model as DM
    r = DM.compose(cfg, packets, dns_on=dns_on, control_kinds=control_kinds, tunnel_kinds=tunnel_kinds)
    for lvl in r["levels"]:
        for part in lvl:
            c = dict(cfg, first=part["first"])
            ref = part["results"]
            d = tls(c, part["data"], part["offsets"], part["caplens"], ref["records"], ref["layouts"],
                    ref["err_args"]) if tls_on else None
            part["tls"] = d
            if d is None:
                continue
            for i, g in enumerate(part["origin"]):
                v = int(d["verdict"][i])
                if v < 0:
                    continue
                t = d["records"][v]
                r["truncated"][g] = r["truncated"][g] or bool(t["status"] & 1)
                if t["err"]:
                    r["error"][g] = error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"]))
                else:
                    r["decoded"][g] = r["decoded"][g] + [LT_TLS]
                    r["error"][g] = ""
    return r
