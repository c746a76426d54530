"""Executable statement of the UDP service rules (include/gpk_svc.h, DESIGN.md
§28), independent of the C++ in gopacket_amd/csrc/gpk_svc_rules.h.

  decode_dhcp4_option   DHCPOption.decode, dhcpv4.go:563-583
  decode_dhcp4          DHCPv4.DecodeFromBytes, dhcpv4.go:126-184
  decode_dhcp6_option   DHCPv6Option.decode, dhcpv6_options.go:611-622, the
                        uint16 sum of :618 and :620 included
  decode_dhcp6          DHCPv6.DecodeFromBytes, dhcpv6.go:89-124
  decode_ntp            NTP.DecodeFromBytes, ntp.go:294-347
                        on Go-style slices, loop for loop as the reference
                        writes them, every message into a fresh struct
  svc_packet            the candidate rule, then the layer
  svc(cfg, ...)         gpk_svc_batch's outputs, the capacity rule included
  compose(base, ...)    DecodeLayers with the three layers added to a parser
                        whose composition without them is `base`

The candidate's payload and next type come from tunnel_model.last_payload.
"""
import numpy as np

import tunnel_model as TM
from tunnel_model import GoPanic, Sl, Tables
from gopacket_amd import _lib

LT_NTP, LT_DHCP4, LT_DHCP6 = 117, 118, 134
LAYER_TYPES = (LT_DHCP4, LT_DHCP6, LT_NTP)
KIND_OF_TYPE = {LT_DHCP4: 1, LT_DHCP6: 2, LT_NTP: 4}
ALL = 7
E_PANIC_SLICE_B = 4
TRUNCATED = (160, 165, 166, 169)
ALL_ERRORS = tuple(range(160, 170)) + (E_PANIC_SLICE_B,)

TEXT = {
    0: "",
    160: "DHCPv4 length %(a0)d too short",
    161: "DHCPv4 hardware address length %(a0)d exceeds 16",
    162: "Bad DHCP header",
    163: "Not enough data to decode",
    164: "Option is malformed",
    165: "DHCPv6 length %(a0)d too short",
    166: "DHCPv6 length %(a0)d too short for message type %(a1)d",
    167: "not enough data to decode",
    168: "dhcpv6 option size < length %(a0)d",
    169: "NTP packet too short",
    E_PANIC_SLICE_B: "panic: runtime error: slice bounds out of range [%(a0)d:%(a1)d]",
}


class GoError(Exception):
    def __init__(self, code, a0=0, a1=0):
        Exception.__init__(self, code, a0, a1)
        self.code, self.a0, self.a1 = code, a0, a1


def error_text(code, a0=0, a1=0):
    return TEXT[code] % dict(a0=a0, a1=a1)


def u16(x):
    return x & 0xffff


def decode_dhcp4_option(d):
    """(Type, Length, Data slice or None) of DHCPOption.decode into a fresh DHCPOption."""
    if d.len < 1:
        raise GoError(163)
    typ, length, data = d[0], 0, None
    if typ not in (0, 255):
        if d.len < 2:
            raise GoError(163)
        length = d[1]
        if length > d.sl(2).len:
            raise GoError(164)
        data = d.sl(2, 2 + length)
    return typ, length, data


def decode_dhcp4(d):
    if d.len < 240:
        raise GoError(160, d.len)
    hlen = d[2]
    if hlen > 16:
        raise GoError(161, hlen)
    r = dict(b=[d[0], d[1], hlen, d[3]],
             v=[d.be32(4), d.be16(8) | d.be16(10) << 16] + [int.from_bytes(d.sl(12 + 4 * k, 16 + 4 * k).bytes(), "little")
                                                           for k in range(4)],
             entries=[], contents_len=0)
    d.sl(28, 28 + hlen), d.sl(44, 108), d.sl(108, 236)
    if d.be32(236) != 0x63825363:
        raise GoError(162)
    if d.len <= 240:
        return r  # Contents is not set
    options = d.sl(240)
    stop, start = options.len, 0
    while start < stop:
        typ, length, data = decode_dhcp4_option(options.sl(start))
        if typ == 255:
            break
        # a Pad has no Data: its descriptor names the offset behind its byte
        r["entries"].append(dict(code=typ, length=length, off=data.off if data is not None else options.off + start + 1))
        start += 1 if typ == 0 else length + 2
    r["contents_len"] = d.len
    return r


def decode_dhcp6_option(d):
    """(Code, Length, Data slice) of DHCPv6Option.decode."""
    if d.len < 4:
        raise GoError(167)
    code, length = d.be16(0), d.be16(2)
    if d.len < 4 + length:
        raise GoError(168, u16(4 + length))
    return code, length, d.sl(4, u16(4 + length))  # the high bound is a uint16 sum: below 4 it panics


def decode_dhcp6(d):
    if d.len < 4:
        raise GoError(165, d.len)
    typ = d[0]
    r = dict(b=[typ, 0, 0, 0], v=[0] * 6, entries=[], contents_len=d.len)
    if typ in (12, 13):
        if d.len < 34:
            raise GoError(166, d.len, typ)
        r["b"][1] = d[1]
        r["v"][1], r["v"][2] = d.sl(2, 18).off, d.sl(18, 34).off
        offset = 34
    else:
        r["v"][0] = int.from_bytes(d.sl(1, 4).bytes(), "big")
        offset = 4
    stop = d.len
    while offset < stop:
        code, length, data = decode_dhcp6_option(d.sl(offset))
        r["entries"].append(dict(code=code, length=length, off=data.off))
        offset += length + 4
    return r


def decode_ntp(d):
    if d.len < 48:
        raise GoError(169)
    f = d[0]
    ext = d.sl(48)
    for k in range(4):
        d.sl(16 + 8 * k, 24 + 8 * k)  # the four timestamps: read from the packet, not part of the record
    return dict(b=[(f & 0xC0) >> 6, (f & 0x38) >> 3, f & 7, d[1]],
                v=[d[2] | d[3] << 8, d.be32(4), d.be32(8), d.be32(12), ext.off, ext.len], entries=[], contents_len=d.len)


DECODERS = {LT_DHCP4: decode_dhcp4, LT_DHCP6: decode_dhcp6, LT_NTP: decode_ntp}


def decode_message(lt, d):
    """(class, record dict with "entries") of the layer lt over the slice d."""
    t = dict(layer_type=lt, hdr_off=d.off, _len=d.len)  # _len: the slice handed in (no field of the record)
    try:
        r = DECODERS[lt](d)
    except GoError as e:
        t.update(err=e.code, err_a0=e.a0, err_a1=e.a1, status=1 if e.code in TRUNCATED else 0, entries=[])
        return _lib.SVC_CLASS_FAILED, t
    except GoPanic as e:
        assert e.code == E_PANIC_SLICE_B, e  # the one panic of the path: data[4 : 4+o.Length]
        t.update(err=e.code, err_a0=e.a0, err_a1=e.a1, status=0, entries=[])
        return _lib.SVC_CLASS_FAILED, t
    t.update(r, len=d.len, nentries=len(r["entries"]))
    return _lib.SVC_CLASS_OK, t


def svc_packet(T, pkt, rec, lay, kinds):
    """One packet: (class or SVC_NONE / SVC_UNKNOWN, record dict or None)."""
    status = int(rec["status"])
    nl = (status >> 8) & 0xfff
    if nl > 16:
        return _lib.SVC_UNKNOWN, None
    err = status & 0x7f
    if nl == 0 or err not in (0, 1):
        return _lib.SVC_NONE, None
    dec = TM.CODE_DEC[(int(rec["layers"]) >> (4 * (nl - 1))) & 15]
    if dec in ("PAYLOAD", "FRAGMENT"):
        return _lib.SVC_NONE, None
    k = TM.SLOTS.index(dec)
    off, ln, nxt = TM.last_payload(T, dec, pkt, int(lay["start"][k]), int(lay["end"][k]))
    if ln == 0 or not KIND_OF_TYPE.get(nxt, 0) & kinds:
        return _lib.SVC_NONE, None
    return decode_message(nxt, Sl(pkt, off, ln, len(pkt) - off))


def _row(dt, t):
    row = np.zeros(1, dt)
    for name in dt.names:
        if name in t:
            row[name] = t[name]
    return row[0]


def svc(cfg, data, offsets, caplens, records, layouts, kinds=ALL, entry_cap=0, fill=0):
    """gpk_svc_batch's outputs (arrays start as `fill` bytes)."""
    T = Tables(cfg)
    n = len(caplens)
    raw = bytes(np.ascontiguousarray(data, np.uint8))
    res = []
    for i in range(n):
        o, c = int(offsets[i]), int(caplens[i])
        res.append(svc_packet(T, raw[o:o + c], records[i], layouts[i], kinds))

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(verdict=arr(n, np.int32), class_start=arr(3, np.uint32), index=arr(n, np.uint32),
               records=arr(n, _lib.SVC_DTYPE), counts=arr(8, np.uint32), entries=arr(entry_cap, _lib.SVC_ENTRY_DTYPE))
    j = total = 0
    for c in range(_lib.SVC_NCLASS):
        out["class_start"][c] = j
        for i, (cls, t) in enumerate(res):
            if cls != c:
                continue
            out["verdict"][i] = j
            out["index"][j] = i
            rec = _row(_lib.SVC_DTYPE, t)
            if c == _lib.SVC_CLASS_OK:
                rec["entry0"] = total
                ents = t["entries"]
                if ents and total + len(ents) > entry_cap:
                    rec["status"] |= _lib.SVC_ST_DROPPED
                else:
                    for q, e in enumerate(ents):
                        out["entries"][total + q] = _row(_lib.SVC_ENTRY_DTYPE, e)
                total += len(ents)
            out["records"][j] = rec
            j += 1
    out["class_start"][2] = j
    for i, (cls, t) in enumerate(res):
        if cls < 0:
            out["verdict"][i] = cls
    out["counts"][:] = 0
    out["counts"][0] = j
    out["counts"][1:3] = np.diff(out["class_start"].astype(np.int64))
    if j:
        out["counts"][3] = total > entry_cap
        out["counts"][4], out["counts"][5] = total & 0xffffffff, total >> 32
    return out


def compose(cfg, packets, kinds=ALL, base=None, tunnel_kinds=0):
    """DecodeLayers of every packet with the layers `kinds` added to a parser
    of `cfg`. base: that parser's composition without them (control_model's,
    ndp_model's or tunnel_model's dict; default tunnel_model's with
    tunnel_kinds): this pass then runs over every level's part. Returns the
    dict; every level entry gains "svc"."""
    r = base if base is not None else TM.compose(cfg, packets, kinds=tunnel_kinds)
    for lvl in r["levels"]:
        for part in lvl:
            c = dict(cfg, first=part["first"])
            ref = part["results"]
            need = svc(c, part["data"], part["offsets"], part["caplens"], ref["records"], ref["layouts"], kinds, 0)
            cap = int(need["counts"][4])
            sv = svc(c, part["data"], part["offsets"], part["caplens"], ref["records"], ref["layouts"], kinds, cap)
            part["svc"] = sv
            for i, g in enumerate(part["origin"]):
                v = int(sv["verdict"][i])
                if v < 0:
                    continue
                t = sv["records"][v]
                r["truncated"][g] = r["truncated"][g] or bool(t["status"] & 1)
                if t["err"]:
                    r["error"][g] = error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"]))
                else:
                    r["decoded"][g].append(int(t["layer_type"]))
                    r["error"][g] = ""
    return r
