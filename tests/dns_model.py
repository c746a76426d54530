"""Executable statement of the DNS rules (include/gpk_dns.h),
independent of the C++ in gopacket_amd/csrc/gpk_dns_rules.h: layers/dns.go's
decode restated on Go-style slices, recursion and all.

  decode_name           decodeName, dns.go:814-920 (recursive, as written)
  decode_question       DNSQuestion.decode, :933-952
  decode_record         DNSResourceRecord.decode, :1056-1087
  decode_rdata          decodeRData, :1350-1529, with decodeCharacterStrings
                        (:1267-1278), decodeOPTs (:1280-1307), decodeSVCB
                        (:1309-1348), DNSRRSIG.decode (:1726-1748) and
                        DNSKEY.decode (:1815-1824)
  decode_message        DNS.DecodeFromBytes, :333-421
  dns_packet            the candidate rule, then decode_message
  dns(cfg, ...)         gpk_dns_batch's outputs
  compose(cfg, packets) DecodeLayers with layers.DNS (and, optionally, the
                        control and tunnel layers) added to the parser of `cfg`

The candidate's payload and next type come from tunnel_model.last_payload, and
the six-layer decode of every level is the oracle's (oracle/).
"""
import sys

import numpy as np

import tunnel_model as TM
from tunnel_model import Tables
from gopacket_amd import _lib

LT_DNS = 107
(E_SHORT, E_MAXREC, E_OFFHIGH, E_LONG, E_INVIDX, E_PTRHIGH, E_RANGE, E_Q40, E_Q80, E_QSMALL, E_RSMALL, E_RLEN,
 E_CHARSTR, E_SOA, E_MX, E_URI, E_SRV, E_NAPTR, E_NF_MISS, E_NF_TRUNC, E_NS_MISS, E_NS_TRUNC, E_NR_MISS, E_NR_TRUNC,
 E_OPT_LEN, E_OPT_MAL, E_OPT_IMPL, E_SVCB_LEN, E_SVCB_TRUNC, E_RRSIG, E_DNSKEY) = range(90, 121)
ALL_ERRORS = tuple(range(90, 121))
TEXT = {
    E_SHORT: "DNS packet too short", E_MAXREC: "max DNS recursion level hit", E_OFFHIGH: "dns name offset too high",
    E_LONG: "dns name is too long", E_INVIDX: "dns name uncomputable: invalid index",
    E_PTRHIGH: "dns offset pointer too high", E_RANGE: "dns index walked out of range",
    E_Q40: "qname '0x40' - RFC 2673 unsupported yet (data=%x index=%d)",
    E_Q80: "qname '0x80' unsupported yet (data=%x index=%d)", E_QSMALL: "DNS question too small",
    E_RSMALL: "DNS record too small", E_RLEN: "resource record length exceeds data",
    E_CHARSTR: "Insufficient data for a <character-string>", E_SOA: "SOA too small", E_MX: "MX too small",
    E_URI: "URI too small", E_SRV: "SRV too small", E_NAPTR: "NAPTR too small", E_NF_MISS: "NAPTR Flags missing",
    E_NF_TRUNC: "NAPTR Flags truncated", E_NS_MISS: "NAPTR Service missing", E_NS_TRUNC: "NAPTR Service truncated",
    E_NR_MISS: "NAPTR Regexp missing", E_NR_TRUNC: "NAPTR Regexp truncated",
    E_OPT_LEN: "DNSOPT record is of length %d, it should be at least length 4",
    E_OPT_MAL: "Malformed DNSOPT record.  Length %d < %d",
    E_OPT_IMPL: "Malformed DNSOPT record. The length (%d) field implies a packet larger than the one received",
    E_SVCB_LEN: "DNSSVCB record is of length %d, it should be at least length 3",
    E_SVCB_TRUNC: "DNSSVCB record truncated in SvcParams", E_RRSIG: "RRSIG too small", E_DNSKEY: "DNSKEY too small"}


class GoError(Exception):
    def __init__(self, code, a0=0, a1=0):
        Exception.__init__(self, code, a0, a1)
        self.code, self.a0, self.a1 = code, a0, a1


def error_text(code, a0=0, a1=0):
    if code == 0:
        return ""
    t = TEXT[code]
    k = t.count("%")
    return t % ((a0, a1)[:k]) if k else t


def be16(d, i):
    return d[i] << 8 | d[i + 1]


def be32(d, i):
    return be16(d, i) << 16 | be16(d, i + 2)


def decode_name(data, offset, buffer, level):
    """dns.go:814-920. data: bytes (the Go slice); buffer: a bytearray that
    the name is appended to. Returns (name bytes, index after the name)."""
    if level > 255:
        raise GoError(E_MAXREC)
    elif offset >= len(data):
        raise GoError(E_OFFHIGH)
    start = len(buffer)
    index = offset
    if data[index] == 0:
        return b"", index + 1
    while data[index] != 0:
        form = data[index] & 0xc0
        if form == 0xc0:
            if index + 2 > len(data):
                raise GoError(E_PTRHIGH)
            offsetp = be16(data, index) & 0x3fff
            if offsetp > len(data):
                raise GoError(E_PTRHIGH)
            decode_name(data, offsetp, buffer, level + 1)
            index += 1
            break
        elif form == 0x40:
            raise GoError(E_Q40, data[index], index)
        elif form == 0x80:
            raise GoError(E_Q80, data[index], index)
        else:
            index2 = index + data[index] + 1
            if index2 - offset > 255:
                raise GoError(E_LONG)
            elif index2 > len(data):
                raise GoError(E_INVIDX)
            buffer += b"."
            buffer += data[index + 1:index2]
            index = index2
        if index >= len(data):
            raise GoError(E_RANGE)
    if len(buffer) <= start:
        return bytes(buffer[start:]), index + 1
    return bytes(buffer[start + 1:]), index + 1


def decode_question(data, offset, buffer):
    name, endq = decode_name(data, offset, buffer, 1)
    if len(data) < endq + 4:
        raise GoError(E_QSMALL)
    return dict(section=0, name=name, type=be16(data, endq), cls=be16(data, endq + 2)), endq + 4


def character_strings(d):
    n, index, end = 0, 0, len(d)
    while index != end:
        index2 = index + 1 + d[index]
        if index2 > end:
            raise GoError(E_CHARSTR)
        n += 1
        index = index2
    return n


def decode_opts(data, offset):
    end = len(data)
    if offset == end:
        return 0
    if offset + 4 > end:
        raise GoError(E_OPT_LEN, end - offset)
    n, i = 0, offset
    while i < end:
        if len(data) < i + 4:
            raise GoError(E_OPT_MAL, len(data), i + 4)
        ln = be16(data, i + 2)
        if i + 4 + ln > end:
            raise GoError(E_OPT_IMPL, ln)
        n += 1
        i += ln + 4
    return n


def decode_rdata(rr, data, offset, buffer, base):
    """decodeRData on data = message[:end]; base: packet offset of the message."""
    t = rr["type"]
    v = rr["v"]
    dl = rr["data_length"]
    if t in (16, 13):
        rr["count"] = character_strings(data[offset:offset + dl])
    elif t in (2, 5, 12):
        rr["rname"], _ = decode_name(data, offset, buffer, 1)
    elif t == 6:
        rr["rname"], endq = decode_name(data, offset, buffer, 1)
        name, endq = decode_name(data, endq, buffer, 1)
        if len(data) < endq + 20:
            raise GoError(E_SOA)
        rr["rname2"] = name
        v[0:5] = [be32(data, endq + 4 * k) for k in range(5)]
    elif t == 15:
        if len(data) < offset + 2:
            raise GoError(E_MX)
        v[0] = be16(data, offset)
        rr["rname"], _ = decode_name(data, offset + 2, buffer, 1)
    elif t == 256:
        if dl < 4:
            raise GoError(E_URI)
        v[0], v[1] = be16(data, offset), be16(data, offset + 2)
    elif t == 33:
        if len(data) < offset + 6:
            raise GoError(E_SRV)
        v[0], v[1], v[2] = be16(data, offset), be16(data, offset + 2), be16(data, offset + 4)
        rr["rname"], _ = decode_name(data, offset + 6, buffer, 1)
    elif t == 35:
        if len(data) < offset + 4:
            raise GoError(E_NAPTR)
        v[0], v[1] = be16(data, offset), be16(data, offset + 2)
        offset += 4
        for k, (miss, trunc) in enumerate(((E_NF_MISS, E_NF_TRUNC), (E_NS_MISS, E_NS_TRUNC), (E_NR_MISS, E_NR_TRUNC))):
            if len(data) < offset + 1:
                raise GoError(miss)
            ln = data[offset]
            offset += 1
            if len(data) < offset + ln:
                raise GoError(trunc)
            v[2 + 2 * k], v[3 + 2 * k] = base + offset, ln
            offset += ln
        rr["rname"], _ = decode_name(data, offset, buffer, 1)
    elif t == 41:
        rr["count"] = decode_opts(data, offset)
    elif t == 46:
        if len(data) < offset + 18:
            raise GoError(E_RRSIG)
        v[0], v[1], v[2] = be16(data, offset), data[offset + 2], data[offset + 3]
        v[3], v[4], v[5] = be32(data, offset + 4), be32(data, offset + 8), be32(data, offset + 12)
        v[6] = be16(data, offset + 16)
        signer = bytearray()  # its own buffer (:1739), then the strip of :1740-1742
        _, end = decode_name(data, offset + 18, signer, 1)
        if len(signer) > 1:
            signer = signer[1:]
        rr["rname"] = bytes(signer)
        v[7], v[8] = base + end, len(data) - end
    elif t == 48:
        if len(data) < offset + 4:
            raise GoError(E_DNSKEY)
        v[0], v[1], v[2] = be16(data, offset), data[offset + 2], data[offset + 3]
    elif t in (64, 65):
        end = len(data)
        assert offset != end  # "DNSSVCB record is empty": DataLength > 0 here
        if offset + 3 > end:
            raise GoError(E_SVCB_LEN, end - offset)
        v[0] = be16(data, offset)
        rr["rname"], ofs = decode_name(data, offset + 2, buffer, 1)
        v[1] = base + ofs
        while ofs < end:
            if ofs + 4 > end:
                raise GoError(E_SVCB_TRUNC)
            ln = be16(data, ofs + 2)
            if ofs + 4 + ln > end:
                raise GoError(E_SVCB_TRUNC)
            rr["count"] += 1
            ofs += 4 + ln


def decode_record(data, offset, buffer, section, base):
    name, endq = decode_name(data, offset, buffer, 1)
    if len(data) < endq + 10:
        raise GoError(E_RSMALL)
    rr = dict(section=section, name=name, type=be16(data, endq), cls=be16(data, endq + 2), ttl=be32(data, endq + 4),
              data_length=be16(data, endq + 8), data_off=base + endq + 10, count=0, v=[0] * 10)
    end = endq + 10 + rr["data_length"]
    if end > len(data):
        raise GoError(E_RLEN)
    if rr["data_length"] > 0:
        decode_rdata(rr, data[:end], endq + 10, buffer, base)
    return rr, end


def decode_message(data, base=0):
    """DNS.DecodeFromBytes: the message dict (with "rrs", a list of entry
    dicts whose names are bytes); raises GoError."""
    if len(data) < 12:
        raise GoError(E_SHORT)
    m = dict(len=len(data), id=be16(data, 0), flags2=data[2], flags3=data[3], response_code=data[3] & 0xf,
             qdcount=be16(data, 4), ancount=be16(data, 6), nscount=be16(data, 8), arcount=be16(data, 10), rrs=[])
    buffer = bytearray()
    offset = 12
    for _ in range(m["qdcount"]):
        q, offset = decode_question(data, offset, buffer)
        m["rrs"].append(q)
    for section, count in ((1, m["ancount"]), (2, m["nscount"]), (3, m["arcount"])):
        for _ in range(count):
            rr, offset = decode_record(data, offset, buffer, section, base)
            m["rrs"].append(rr)
            if section == 3 and rr["type"] == 41:
                m["response_code"] = (m["response_code"] | (rr["ttl"] >> 20 & 0xf0)) & 0xff
    return m


def dns_packet(T, pkt, rec, lay, err_a0):
    """One packet: (class or DNS_NONE / DNS_UNKNOWN, message dict or None)."""
    status = int(rec["status"])
    nl = (status >> 8) & 0xfff
    if nl > 16:
        return _lib.DNS_UNKNOWN, None
    err = status & 0x7f
    if nl == 0 or err not in (0, 1):
        return _lib.DNS_NONE, None
    dec = TM.CODE_DEC[(int(rec["layers"]) >> (4 * (nl - 1))) & 15]
    if dec in ("PAYLOAD", "FRAGMENT"):
        return _lib.DNS_NONE, None
    k = TM.SLOTS.index(dec)
    off, ln, nxt = TM.last_payload(T, dec, pkt, int(lay["start"][k]), int(lay["end"][k]))
    if err == 1 and err_a0 is not None:
        assert nxt == err_a0, (nxt, err_a0)
    if nxt != LT_DNS or ln == 0:
        return _lib.DNS_NONE, None
    try:
        m = decode_message(pkt[off:off + ln], off)
    except GoError as e:
        return _lib.DNS_CLASS_FAILED, dict(err=e.code, err_a0=e.a0, err_a1=e.a1, hdr_off=off,
                                           status=1 if e.code == E_SHORT else 0, rrs=[])
    m["hdr_off"] = off
    return _lib.DNS_CLASS_OK, m


def dns(cfg, data, offsets, caplens, records, layouts, err_args=None, rr_cap=None, name_cap=None, fill=0):
    """gpk_dns_batch's outputs (arrays start as `fill` bytes). rr_cap /
    name_cap None: exactly what the batch needs."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
    T = Tables(cfg)
    n = len(caplens)
    raw = bytes(np.ascontiguousarray(data, np.uint8))
    res = []
    for i in range(n):
        o, c = int(offsets[i]), int(caplens[i])
        a0 = int(err_args[2 * i]) if err_args is not None else None
        if a0 is not None and a0 >= 1 << 31:
            a0 -= 1 << 32
        res.append(dns_packet(T, raw[o:o + c], records[i], layouts[i], a0))
    need_rr = sum(len(m["rrs"]) for c, m in res if c == 0)
    need_nb = sum(len(r["name"]) + len(r.get("rname", b"")) + len(r.get("rname2", b""))
                  for c, m in res if c == 0 for r in m["rrs"])
    rr_cap = need_rr if rr_cap is None else rr_cap
    name_cap = need_nb if name_cap is None else name_cap

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(verdict=arr(n, np.int32), class_start=arr(3, np.uint32), index=arr(n, np.uint32),
               records=arr(n, _lib.DNS_DTYPE), counts=arr(8, np.uint32), rrs=arr(rr_cap, _lib.DNS_RR_DTYPE),
               names=arr(name_cap, np.uint8))
    j = rr0 = name0 = 0
    for c in range(_lib.DNS_NCLASS):
        out["class_start"][c] = j
        for i, (cls, m) in enumerate(res):
            if cls != c:
                continue
            out["verdict"][i] = j
            out["index"][j] = i
            rec = np.zeros(1, _lib.DNS_DTYPE)
            rec["kind"] = 1
            for name in _lib.DNS_DTYPE.names:
                if name in m:
                    rec[name] = m[name]
            if c == 0:
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
                rec["nrr"], rec["name_bytes"], rec["rr0"], rec["name0"] = len(rows), len(blob), rr0, name0
                if rr0 + len(rows) <= rr_cap and name0 + len(blob) <= name_cap:
                    for k, row in enumerate(rows):
                        out["rrs"][rr0 + k] = row
                    out["names"][name0:name0 + len(blob)] = np.frombuffer(bytes(blob), np.uint8)
                else:
                    rec["status"] |= _lib.DNS_ST_DROPPED
                rr0 += len(rows)
                name0 += len(blob)
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
        out["counts"][3] = int(need_rr > rr_cap or need_nb > name_cap)
        out["counts"][4], out["counts"][5] = need_rr & 0xffffffff, need_rr >> 32
        out["counts"][6], out["counts"][7] = need_nb & 0xffffffff, need_nb >> 32
    assert (rr0, name0) == (need_rr, need_nb)
    return out


def messages(out):
    """The OK messages of dns() / DNSDecoder outputs as (packet index, record, entry dicts with
    the names as bytes): for comparisons by value."""
    res = []
    for j in range(int(out["class_start"][0]), int(out["class_start"][1])):
        rec = out["records"][j]
        rows = []
        for k in range(int(rec["rr0"]), int(rec["rr0"]) + int(rec["nrr"])):
            r = out["rrs"][k]
            name = lambda o, l: bytes(out["names"][int(r[o]):int(r[o]) + int(r[l])])  # noqa: E731
            rows.append(dict(section=int(r["section"]), type=int(r["type"]), cls=int(r["cls"]), ttl=int(r["ttl"]),
                             name=name("name_off", "name_len"), rname=name("rname_off", "rname_len"),
                             rname2=name("rname2_off", "rname2_len"), count=int(r["count"]),
                             v=[int(x) for x in r["v"]]))
        res.append((int(out["index"][j]), rec, rows))
    return res


def compose(cfg, packets, dns_on=True, control_kinds=0, tunnel_kinds=0):
    """DecodeLayers of every packet with layers.DNS (and the control layers
    `control_kinds`, the tunnel layers `tunnel_kinds`) added to the parser of
    `cfg`: control_model's composition, then the DNS pass over every level's
    part. A DNS candidate's last layer leads to LayerTypeDNS, so it is neither
    a tunnel nor a control candidate. Every level entry gains "dns"."""
    import control_model as CM
    r = CM.compose(cfg, packets, kinds=control_kinds, tunnel_kinds=tunnel_kinds) if control_kinds else \
        TM.compose(cfg, packets, kinds=tunnel_kinds)
    for lvl in r["levels"]:
        for part in lvl:
            c = dict(cfg, first=part["first"])
            ref = part["results"]
            d = dns(c, part["data"], part["offsets"], part["caplens"], ref["records"], ref["layouts"],
                    ref["err_args"]) if dns_on else None
            part["dns"] = d
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
                    r["decoded"][g] = r["decoded"][g] + [LT_DNS]
                    r["error"][g] = ""
    return r
