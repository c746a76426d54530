"""Executable statement of the NDP / MLD rules (include/gpk_ndp.h, DESIGN.md
§27), independent of the C++ in gopacket_amd/csrc/gpk_ndp_rules.h.

  decode_options        ICMPv6Options.DecodeFromBytes, icmp6msg.go:514-546
  decode_*              DecodeFromBytes of the ten layers (icmp6msg.go:190-202,
                        237-255, 306-319, 355-369, 422-436, mldv1.go:32-43,
                        95-106, mldv2.go:61-90, 309-333, 473-509) on Go-style
                        slices, loop for loop as the reference writes them
  ndp_packet            the candidate rule's two ways in, then the layer
  ndp(cfg, ...)         gpk_ndp_batch's outputs, the capacity rule included
  compose(cfg, packets) DecodeLayers with the control layers, the ten message
                        layers (and, optionally, the tunnel layers) added to
                        the parser of `cfg`

The candidate's payload and next type come from tunnel_model.last_payload, the
ICMPv6 header in front from control_model.
"""
import numpy as np

import control_model as CM
import tunnel_model as TM
from tunnel_model import Sl, Tables
from gopacket_amd import _lib

(LT_RS, LT_RA, LT_NS, LT_NA, LT_REDIRECT) = range(124, 129)
LT_MLD1_REPORT, LT_MLD1_DONE, LT_MLD1_QUERY, LT_MLD2_REPORT, LT_MLD2_QUERY = range(135, 140)
KIND_OF_TYPE = {LT_RS: 1, LT_RA: 2, LT_NS: 4, LT_NA: 8, LT_REDIRECT: 16, LT_MLD1_QUERY: 32, LT_MLD1_REPORT: 64,
                LT_MLD1_DONE: 128, LT_MLD2_QUERY: 256, LT_MLD2_REPORT: 512}
ICMP6 = 1024
ALL = 2047
NOT_TRUNCATED = (154,)

TEXT = {
    0: "",
    140: "ICMP layer less then 4 bytes for ICMPv6 router solicitation",
    141: "ICMP layer less then 12 bytes for ICMPv6 router advertisement",
    142: "ICMP layer less then 20 bytes for ICMPv6 neighbor solicitation",
    143: "ICMP layer less then 20 bytes for ICMPv6 neighbor advertisement",
    144: "ICMP layer less then 36 bytes for ICMPv6 redirect",
    145: "ICMP layer less then 2 bytes for ICMPv6 message option",
    146: "ICMPv6 message option with length 0",
    147: "ICMP layer only %(a0)d bytes for ICMPv6 message option with length %(a1)d",
    148: "ICMP layer less than 20 bytes for Multicast Listener Query Message V1",
    149: "ICMP layer less than 24 bytes for Multicast Listener Query Message V2",
    150: "ICMP layer less than %(a0)d bytes for Multicast Listener Query Message V2",
    151: "ICMP layer less than 4 bytes for Multicast Listener Report Message V2",
    152: "Multicast Listener Report Message V2 layer less than 4 bytes for Multicast Address Record",
    153: "Multicast Listener Report Message V2 layer less than %(a0)d bytes for Multicast Address Record",
    154: "Multicast Listener Report Message V2 layer less than %(a0)d bytes for Multicast Address Record",
}


class GoError(Exception):
    def __init__(self, code, a0=0, a1=0):
        Exception.__init__(self, code, a0, a1)
        self.code, self.a0, self.a1 = code, a0, a1


def error_text(code, a0=0, a1=0):
    return TEXT[code] % dict(a0=a0, a1=a1)


def decode_options(d):
    """The options as (Type, Data slice)."""
    opts = []
    while d.len > 0:
        if d.len < 2:
            raise GoError(145)
        length = d[1] * 8
        if length == 0:
            raise GoError(146)
        if d.len < length:
            raise GoError(147, d.len, length)
        opts.append((d[0], d.sl(2, length)))
        d = d.sl(length)
    return opts


def _options_entries(opts):
    return [dict(type=t, off=s.off, ext=s.len) for t, s in opts]


def decode_rs(d):
    if d.len < 4:
        raise GoError(140)
    return dict(entries=_options_entries(decode_options(d.sl(4))))


def decode_ra(d):
    if d.len < 12:
        raise GoError(141)
    return dict(v=[d.be32(4), d.be32(8), d.be16(2), d[0]], flags=d[1], contents_len=d.len,
                entries=_options_entries(decode_options(d.sl(12))))


def decode_ns(d):
    if d.len < 20:
        raise GoError(142)
    return dict(v=[d.sl(4, 20).off, 0, 0, 0], contents_len=d.len, entries=_options_entries(decode_options(d.sl(20))))


def decode_na(d):
    if d.len < 20:
        raise GoError(143)
    return dict(v=[d.sl(4, 20).off, 0, 0, 0], flags=d[0], contents_len=d.len,
                entries=_options_entries(decode_options(d.sl(20))))


def decode_redirect(d):
    if d.len < 36:
        raise GoError(144)
    return dict(v=[d.sl(4, 20).off, d.sl(20, 36).off, 0, 0], contents_len=d.len,
                entries=_options_entries(decode_options(d.sl(36))))


def decode_mld1(d, query=False):
    if d.len < 20:
        raise GoError(148)
    r = dict(v=[d.sl(4, 20).off, 0, d.be16(0), 0], entries=[])
    if query and d.len > 20:
        p = d.sl(20)
        r.update(payload_off=p.off, payload_len=p.len)
    return r


def decode_mld2_query(d):
    if d.len < 24:
        raise GoError(149)
    n = d.be16(22)
    for i in range(n):
        end = 24 + i * 16 + 16
        if end > d.len:
            raise GoError(150, end)
    return dict(v=[d.sl(4, 20).off, 0, d.be16(0), 0], s_qrv=d[20] & 0xF, qqic=d[21], count=n, entries=[])


def decode_record(d):
    """(entry, bytes read) of MLDv2MulticastAddressRecord.decode."""
    if d.len < 20:
        raise GoError(152)
    aux, n = d[1], d.be16(2)
    for i in range(n):
        end = 20 + i * 16 + 16
        if d.len < end:
            raise GoError(153, end)
    without = 20 + n * 16
    total = aux * 4 + without
    if d.len < total:
        raise GoError(154, without)
    return dict(type=d[0], aux_data_len=aux, n=n, off=d.sl(4, 20).off, ext=d.sl(20, without).off,
                aux_off=d.sl(without, total).off), total


def decode_mld2_report(d):
    if d.len < 4:
        raise GoError(151)
    count = d.be16(2)
    begin, entries = 4, []
    for _ in range(count):
        e, read = decode_record(d.sl(begin))
        entries.append(e)
        begin += read
    return dict(count=count, entries=entries)


DECODERS = {LT_RS: decode_rs, LT_RA: decode_ra, LT_NS: decode_ns, LT_NA: decode_na, LT_REDIRECT: decode_redirect,
            LT_MLD1_QUERY: lambda d: decode_mld1(d, True), LT_MLD1_REPORT: decode_mld1, LT_MLD1_DONE: decode_mld1,
            LT_MLD2_QUERY: decode_mld2_query, LT_MLD2_REPORT: decode_mld2_report}


def decode_message(lt, d):
    """(class, record dict with "entries") of the layer lt over the slice d."""
    t = dict(layer_type=lt, hdr_off=d.off, _len=d.len)  # _len: the slice handed in (no field of the record)
    try:
        r = DECODERS[lt](d)
    except GoError as e:
        t.update(err=e.code, err_a0=e.a0, err_a1=e.a1, status=0 if e.code in NOT_TRUNCATED else 1, entries=[])
        return _lib.NDP_CLASS_FAILED, t
    t.update(r, len=d.len, nentries=len(r["entries"]))
    return _lib.NDP_CLASS_OK, t


def ndp_packet(T, pkt, rec, lay, kinds):
    """One packet: (class or NDP_NONE / NDP_UNKNOWN, record dict or None)."""
    status = int(rec["status"])
    nl = (status >> 8) & 0xfff
    if nl > 16:
        return _lib.NDP_UNKNOWN, None
    err = status & 0x7f
    if nl == 0 or err not in (0, 1):
        return _lib.NDP_NONE, None
    dec = TM.CODE_DEC[(int(rec["layers"]) >> (4 * (nl - 1))) & 15]
    if dec in ("PAYLOAD", "FRAGMENT"):
        return _lib.NDP_NONE, None
    k = TM.SLOTS.index(dec)
    off, ln, nxt = TM.last_payload(T, dec, pkt, int(lay["start"][k]), int(lay["end"][k]))
    if ln == 0:
        return _lib.NDP_NONE, None
    d = Sl(pkt, off, ln, len(pkt) - off)
    if nxt == CM.LT_ICMPV6:  # way 1
        if not kinds & ICMP6:
            return _lib.NDP_NONE, None
        try:
            h = CM.decode_icmp6(d)
        except CM.GoError:
            return _lib.NDP_NONE, None
        d, nxt = h["payload"], h["next_type"]
        if d.len == 0:
            return _lib.NDP_NONE, None
    if not KIND_OF_TYPE.get(nxt, 0) & kinds:
        return _lib.NDP_NONE, None
    return decode_message(nxt, d)


def ndp(cfg, data, offsets, caplens, records, layouts, kinds=ALL, entry_cap=0, fill=0):
    """gpk_ndp_batch's outputs (arrays start as `fill` bytes)."""
    T = Tables(cfg)
    n = len(caplens)
    raw = bytes(np.ascontiguousarray(data, np.uint8))
    res = []
    for i in range(n):
        o, c = int(offsets[i]), int(caplens[i])
        res.append(ndp_packet(T, raw[o:o + c], records[i], layouts[i], kinds))

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(verdict=arr(n, np.int32), class_start=arr(3, np.uint32), index=arr(n, np.uint32),
               records=arr(n, _lib.NDP_DTYPE), counts=arr(8, np.uint32), entries=arr(entry_cap, _lib.NDP_ENTRY_DTYPE))
    j = total = 0
    for c in range(_lib.NDP_NCLASS):
        out["class_start"][c] = j
        for i, (cls, t) in enumerate(res):
            if cls != c:
                continue
            out["verdict"][i] = j
            out["index"][j] = i
            rec = np.zeros(1, _lib.NDP_DTYPE)
            for name in _lib.NDP_DTYPE.names:
                if name in t:
                    rec[name] = t[name]
            if c == _lib.NDP_CLASS_OK:
                rec["entry0"] = total
                ents = t["entries"]
                if ents and total + len(ents) > entry_cap:
                    rec["status"] |= _lib.NDP_ST_DROPPED
                else:
                    for q, e in enumerate(ents):
                        row = np.zeros(1, _lib.NDP_ENTRY_DTYPE)
                        for name, val in e.items():
                            row[name] = val
                        out["entries"][total + q] = row[0]
                total += len(ents)
            out["records"][j] = rec[0]
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


def compose(cfg, packets, kinds=ALL, control_kinds=15, checksum=True, tunnel_kinds=0):
    """DecodeLayers of every packet with the control layers, the message layers
    `kinds` (bit 1024 stands for layers.ICMPv6, as control_kinds' bit 2 does)
    and the tunnel layers added to the parser of `cfg`: control_model's
    composition, then this pass over every level's part. Returns its dict;
    every level entry gains "ndp"."""
    r = CM.compose(cfg, packets, control_kinds, checksum, tunnel_kinds) if control_kinds else \
        TM.compose(cfg, packets, kinds=tunnel_kinds)
    for lvl in r["levels"]:
        for part in lvl:
            c = dict(cfg, first=part["first"])
            ref = part["results"]
            need = ndp(c, part["data"], part["offsets"], part["caplens"], ref["records"], ref["layouts"], kinds, 0)
            cap = int(need["counts"][4])
            nd = ndp(c, part["data"], part["offsets"], part["caplens"], ref["records"], ref["layouts"], kinds, cap)
            part["ndp"] = nd
            for i, g in enumerate(part["origin"]):
                v = int(nd["verdict"][i])
                if v < 0:
                    continue
                t = nd["records"][v]
                r["truncated"][g] = r["truncated"][g] or bool(t["status"] & 1)
                if t["err"]:
                    r["error"][g] = error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"]))
                else:
                    r["decoded"][g].append(int(t["layer_type"]))
                    r["error"][g] = ""
    return r
