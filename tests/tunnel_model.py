"""Executable statement of the tunnel rules (include/gpk_tunnel.h).

The three DecodeFromBytes are restated on a Go-style slice (len, cap, bounds
panics with the run-time's texts), independently of the C++ in
gopacket_amd/csrc/gpk_tunnel_rules.h:

  decode_vxlan / decode_gre / decode_geneve   layers/vxlan.go:53-78, gre.go:40-128,
                                              geneve.go:59-119
  gre_verify                                  GRE.VerifyChecksum gre.go:239-250
  peel(cfg, ...)                              one level: candidates, tunnel records, compact
                                              list in class / packet order (gpk_tunnel_batch)
  compose(cfg, packets)                       DecodeLayers with the three layers added to the
                                              parser: decoded, error text, Truncated per packet,
                                              and every level's batch and results

The six-layer decode of every level is the oracle's (oracle/), the yardstick
of gpk_decode_batch.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from gopacket_amd import _lib  # noqa: E402

REG = json.load(open(os.path.join(os.path.dirname(HERE), "gopacket_amd", "registry_gen.json")))
LT_GRE, LT_VXLAN, LT_GENEVE = 18, 116, 120
KIND_OF_TYPE = {LT_GRE: 1, LT_VXLAN: 2, LT_GENEVE: 4}
TYPE_OF_KIND = {1: LT_GRE, 2: LT_VXLAN, 4: LT_GENEVE}
DEC_TYPES = dict(ETHERNET=(17,), DOT1Q=(15,), IPV4=(20,), IPV6=(21,), IPV6_EXT=(46, 47, 48, 49), TCP=(44,), UDP=(45,),
                 PAYLOAD=(2,), FRAGMENT=(3,))
CLASS_OF_DEC = dict(ETHERNET=0, DOT1Q=1, IPV4=2, IPV6=3)
CLASS_TYPE = (17, 15, 20, 21)
# record code -> decoder (layout slot = index in SLOTS)
CODE_DEC = {1: "ETHERNET", 2: "DOT1Q", 3: "IPV4", 4: "IPV6", 5: "IPV6_EXT", 6: "IPV6_EXT", 7: "IPV6_EXT", 8: "IPV6_EXT",
            9: "TCP", 10: "UDP", 11: "PAYLOAD", 12: "FRAGMENT"}
CODE_TYPE = {1: 17, 2: 15, 3: 20, 4: 21, 5: 46, 6: 47, 7: 48, 8: 49, 9: 44, 10: 45, 11: 2, 12: 3}
SLOTS = ("ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP")
MAX_LEVELS = 8


class GoPanic(Exception):
    def __init__(self, code, a0, a1):
        Exception.__init__(self, code, a0, a1)
        self.code, self.a0, self.a1 = code, a0, a1


class GoError(Exception):
    def __init__(self, code, truncated):
        Exception.__init__(self, code)
        self.code, self.truncated = code, truncated


ERR_TEXT = {70: "vxlan packet too small", 71: "GRE packet too small", 72: "GRE packet truncated",
            73: "geneve option too small", 74: "geneve option too small", 75: "geneve packet too short",
            76: "geneve packet too short"}


def error_text(code, a0=0, a1=0):
    if code == 0:
        return ""
    if code == 2:
        return "panic: runtime error: index out of range [%d] with length %d" % (a0, a1)
    if code == 3:
        return "panic: runtime error: slice bounds out of range [:%d] with capacity %d" % (a0, a1)
    if code == 4:
        return "panic: runtime error: slice bounds out of range [%d:%d]" % (a0, a1)
    return ERR_TEXT[code]


class Sl:
    """A Go []byte: a window of `buf` with len and cap."""

    def __init__(self, buf, off, ln, cap):
        self.buf, self.off, self.len, self.cap = buf, off, ln, cap

    def __getitem__(self, i):
        if i >= self.len:
            raise GoPanic(2, i, self.len)
        return self.buf[self.off + i]

    def sl(self, lo=0, hi=None):
        if hi is None:  # data[lo:]
            if lo > self.len:
                raise GoPanic(4, lo, self.len)
            return Sl(self.buf, self.off + lo, self.len - lo, self.cap - lo)
        if hi > self.cap:
            raise GoPanic(3, hi, self.cap)
        if lo > hi:
            raise GoPanic(4, lo, hi)
        return Sl(self.buf, self.off + lo, hi - lo, self.cap - lo)

    def be16(self, lo):
        s = self.sl(lo, lo + 2)
        return s[0] << 8 | s[1]

    def be32(self, lo):
        s = self.sl(lo, lo + 4)
        return s[0] << 24 | s[1] << 16 | s[2] << 8 | s[3]

    def bytes(self):
        return bytes(self.buf[self.off:self.off + self.len])


def decode_vxlan(d):
    if d.len < 8:
        raise GoError(70, False)
    vni = d.sl(4, 7)
    r = dict(kind=2, raw0=d[0], raw1=d[1], vni=vni[0] << 16 | vni[1] << 8 | vni[2], gbp_id=d.be16(2),
             bits=(1 if d[0] & 0x08 else 0) | (2 if d[0] & 0x80 else 0) | (4 if d[1] & 0x40 else 0) |
             (8 if d[1] & 0x80 else 0))
    r["contents"], r["payload"] = d.sl(0, 8), d.sl(8)
    r["ether_next"] = None  # NextLayerType is LayerTypeEthernet
    return r


def decode_gre(d):
    if d.len < 4:
        raise GoError(71, True)

    def require(offset, size):
        if d.len - offset < size:
            raise GoError(72, True)
    r = dict(kind=1, raw0=d[0], raw1=d[1], protocol=d.be16(2), gre_checksum=0, gre_offset=0, gre_key=0, gre_seq=0,
             gre_ack=0, sres=[])
    offset = 4
    if d[0] & 0x80 or d[0] & 0x40:
        require(offset, 4)
        r["gre_checksum"], r["gre_offset"] = d.be16(offset), d.be16(offset + 2)
        offset += 4
    if d[0] & 0x20:
        require(offset, 4)
        r["gre_key"] = d.be32(offset)
        offset += 4
    if d[0] & 0x10:
        require(offset, 4)
        r["gre_seq"] = d.be32(offset)
        offset += 4
    if d[0] & 0x40:
        r["list_rel"] = offset
        while True:
            require(offset, 4)
            af, so, sl = d.be16(offset), d[offset + 2], d[offset + 3]
            require(offset + 4, sl)
            info = d.sl(offset + 4, offset + 4 + sl).bytes()
            offset += 4 + sl
            if af == 0 and sl == 0:
                break
            r["sres"].append(dict(AddressFamily=af, SREOffset=so, SRELength=sl, RoutingInformation=info))
    if d[1] & 0x80:
        require(offset, 4)
        r["gre_ack"] = d.be32(offset)
        offset += 4
    r["contents"], r["payload"] = d.sl(0, offset), d.sl(offset)
    r["ether_next"] = r["protocol"]
    return r


def _geneve_option(d):
    if d.len < 3:
        raise GoError(73, True)
    cls = d.be16(0)
    typ = d[2]
    flags = d[3] >> 5
    length = ((d[3] & 0x1f) * 4 + 4) & 0xff
    if d.len < length:
        raise GoError(74, True)
    return dict(Class=cls, Type=typ, Flags=flags, Length=length, Data=d.sl(4, length).bytes()), length


def decode_geneve(d):
    if d.len < 7:
        raise GoError(75, True)
    vni = d.sl(4, 7)
    r = dict(kind=4, raw0=d[0], raw1=d[1], gn_version=d[0] >> 7, gn_options_length=((d[0] & 0x3f) * 4) & 0xff,
             bits=(1 if d[1] & 0x80 else 0) | (2 if d[1] & 0x40 else 0), protocol=d.be16(2),
             vni=vni[0] << 16 | vni[1] << 8 | vni[2], options=[])
    offset, length = 8, r["gn_options_length"]
    if d.len < length + 7:
        raise GoError(76, True)
    while length > 0:
        opt, ln = _geneve_option(d.sl(offset))
        r["options"].append(opt)
        length -= ln
        offset = (offset + ln) & 0xff  # uint8
    r["contents"] = d.sl(0, offset)
    r["payload"] = d.sl(offset)
    r["ether_next"] = r["protocol"]
    return r


def compute_checksum(data):
    s = 0
    for i in range(0, len(data) - 1, 2):
        s += data[i] << 8 | data[i + 1]
    if len(data) & 1:
        s += data[-1] << 8
    return s & 0xffffffff


def fold(c):
    while c > 0xffff:
        c = (c >> 16) + (c & 0xffff)
    return ~c & 0xffff


def gre_verify(r):
    """(Valid, Correct, Actual) of GRE.VerifyChecksum."""
    existing = r["gre_checksum"]
    correct = fold((compute_checksum(r["contents"].bytes() + r["payload"].bytes()) - existing) & 0xffffffff)
    return (not r["raw0"] & 0x80) or correct == existing, correct, existing


class Tables:
    """The next-layer tables and the container of a parser configuration
    (tests/configs.py dict)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.ethertype = {v: lt for v, lt, _ in REG["ethertype"]}
        self.ipprotocol = {v: lt for v, lt, _ in REG["ipprotocol"]}
        self.tcp = dict(REG["tcp_port_switch"])
        self.tcp.update(dict(REG["tcp_port_override"]))
        self.udp = dict(REG["udp_port_switch"])
        self.udp.update(dict(REG["udp_port_override"]))
        for name, tab in (("ethertype", self.ethertype), ("ipprotocol", self.ipprotocol), ("tcp_port", self.tcp),
                          ("udp_port", self.udp)):
            tab.update({int(k): int(v) for k, v in (cfg.get(name) or {}).items()})
        self.dispatch = {}
        for d in cfg["decoders"]:
            for lt in DEC_TYPES[d]:
                self.dispatch[lt] = d

    def eth(self, v):
        return self.ethertype.get(v, 0)

    def port(self, tab, sport, dport):
        lt = tab.get(dport, 2)
        return tab.get(sport, 2) if lt == 2 else lt


def last_payload(T, dec, pkt, s, e):
    """(offset, length, NextLayerType) of the last decoded layer: the success
    paths of the six DecodeFromBytes."""
    h = pkt[s:e]
    ln = e - s
    be16 = lambda o: h[o] << 8 | h[o + 1]  # noqa: E731
    if dec == "ETHERNET":
        et, plen = be16(12), ln - 14
        if et < 0x0600:
            plen, et = (et if plen >= et else plen), 0
        return s + 14, plen, T.eth(et)
    if dec == "DOT1Q":
        return s + 4, ln - 4, T.eth(be16(2))
    if dec == "IPV4":
        length, hl, ff = be16(2), (h[0] & 15) * 4, be16(6)
        if length == 0:
            length = ln & 0xffff
        ln = min(ln, length)
        return s + hl, ln - hl, 3 if ff & 0x3fff else T.ipprotocol.get(h[9], 0)
    if dec == "IPV6":
        length, nh, poff, plen = be16(4), h[6], 40, ln - 40
        if nh == 0:
            hnh, actual = h[40], h[41] * 8 + 8
            q, jumbo = 2, None
            while q < actual:
                t = h[40 + q]
                al = 1 if t == 0 else h[40 + q + 1] + 2
                if t == 0xC2 and jumbo is None:
                    jumbo = int.from_bytes(h[40 + q + 2:40 + q + 6], "big")
                q += al
            nh = hnh
            if jumbo is not None:
                return s + 40, min(jumbo, plen), T.ipprotocol.get(hnh, 0)
            poff += actual
            plen -= actual
        return s + poff, min(length, plen), T.ipprotocol.get(nh, 0)
    if dec == "IPV6_EXT":
        actual = h[1] * 8 + 8
        return s + actual, ln - actual, T.ipprotocol.get(h[0], 0)
    if dec == "TCP":
        ds = (h[12] >> 4) * 4
        return s + ds, ln - ds, T.port(T.tcp, be16(0), be16(2))
    if dec == "UDP":
        length = be16(4)
        hlen = length if 8 <= length <= ln else ln
        return s + 8, hlen - 8, T.port(T.udp, be16(0), be16(2))
    return e, 0, 0


def peel_packet(T, pkt, rec, lay, err_a0, kinds, gre_checksum):
    """One packet: (class or TUN_NONE / TUN_UNKNOWN, record dict or None)."""
    status = int(rec["status"])
    nl = (status >> 8) & 0xfff
    if nl > 16:
        return _lib.TUN_UNKNOWN, None
    err = status & 0x7f
    if nl == 0 or err not in (0, 1):
        return _lib.TUN_NONE, None
    code = (int(rec["layers"]) >> (4 * (nl - 1))) & 15
    dec = CODE_DEC[code]
    if dec in ("PAYLOAD", "FRAGMENT"):
        return _lib.TUN_NONE, None
    k = SLOTS.index(dec)
    off, ln, nxt = last_payload(T, dec, pkt, int(lay["start"][k]), int(lay["end"][k]))
    if err == 1:  # UnsupportedLayerType names the next type: a second derivation of it
        assert nxt == err_a0, (nxt, err_a0)
    if not (KIND_OF_TYPE.get(nxt, 0) & kinds) or ln == 0:
        return _lib.TUN_NONE, None
    d = Sl(pkt, off, ln, len(pkt) - off)
    t = dict(kind=KIND_OF_TYPE[nxt], hdr_off=off)
    try:
        r = {LT_VXLAN: decode_vxlan, LT_GRE: decode_gre, LT_GENEVE: decode_geneve}[nxt](d)
    except GoError as e:
        t.update(err=e.code, status=1 if e.truncated else 0)
        return _lib.TUN_CLASS_FAILED, t
    except GoPanic as e:
        t.update(err=e.code, err_a0=e.a0, err_a1=e.a1)
        return _lib.TUN_CLASS_FAILED, t
    contents, payload = r.pop("contents"), r.pop("payload")
    en = r.pop("ether_next")
    t.update(contents_len=contents.len, inner_off=payload.off, inner_len=payload.len,
             next_type=17 if en is None else T.eth(en))
    if "sres" in r:
        sres = r.pop("sres")
        t["count"] = len(sres)
        if "list_rel" in r:
            t["list_off"] = off + r.pop("list_rel")
        if gre_checksum:
            valid, correct, _ = gre_verify(dict(r, contents=contents, payload=payload))
            if r["raw0"] & 0x80:
                t.update(gre_correct=correct, status=2 | (4 if valid else 0))
            else:
                t["status"] = 4
        t["model_sres"] = sres
    if "options" in r:
        opts = r.pop("options")
        t.update(count=len(opts), list_off=off + 8, model_options=opts)
    t.update(r)
    if t["inner_len"] == 0:
        return _lib.TUN_CLASS_NOINNER, t
    return CLASS_OF_DEC.get(T.dispatch.get(t["next_type"]), _lib.TUN_CLASS_NOINNER), t


def peel(cfg, data, offsets, caplens, records, layouts, err_args=None, kinds=7, gre_checksum=True, fill=0):
    """gpk_tunnel_batch's outputs (arrays start as `fill` bytes), plus
    "model": the per-entry dicts with the option / SRE lists."""
    T = Tables(cfg)
    n = len(caplens)
    raw = bytes(np.ascontiguousarray(data, np.uint8))
    res = []
    for i in range(n):
        o, c = int(offsets[i]), int(caplens[i])
        a0 = int(err_args[2 * i]) if err_args is not None else None
        cls, t = peel_packet(T, raw[o:o + c], records[i], layouts[i], a0, kinds, gre_checksum)
        res.append((cls, t))

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(verdict=arr(n, np.int32), class_start=arr(7, np.uint32), index=arr(n, np.uint32),
               in_offsets=arr(n, np.uint64), in_caplens=arr(n, np.uint32), tunnels=arr(n, _lib.TUNNEL_DTYPE),
               counts=arr(8, np.uint32), model=[])
    j = 0
    sums = 0
    for c in range(6):
        out["class_start"][c] = j
        for i, (cls, t) in enumerate(res):
            if cls != c:
                continue
            out["verdict"][i] = j
            out["index"][j] = i
            out["in_offsets"][j] = int(offsets[i]) + t.get("inner_off", 0)
            out["in_caplens"][j] = t.get("inner_len", 0)
            rec = np.zeros(1, _lib.TUNNEL_DTYPE)
            for name in _lib.TUNNEL_DTYPE.names:
                if name in t:
                    rec[name] = t[name]
            out["tunnels"][j] = rec[0]
            sums += bool(t.get("status", 0) & 2)
            out["model"].append(t)
            j += 1
    out["class_start"][6] = j
    for i, (cls, t) in enumerate(res):
        if cls < 0:
            out["verdict"][i] = cls
    out["counts"][0] = j
    out["counts"][1:7] = np.diff(out["class_start"].astype(np.int64))
    out["counts"][7] = sums
    return out


def compose(cfg, packets, kinds=7, gre_checksum=True, max_levels=MAX_LEVELS):
    """DecodeLayers of every packet with the tunnel layers added to the parser
    of `cfg`. Returns dict(decoded=[[LayerType]], error=[text], truncated=[bool],
    levels=[dict(packets, origin, first, results, peel)]): level k holds one
    entry per (first layer type) batch, in class order."""
    from oracle import oracle as O
    import configs
    from pktutil import pack
    n = len(packets)
    decoded = [[] for _ in range(n)]
    error = [""] * n
    trunc = [False] * n
    levels = []
    work = [(cfg["first"], list(packets), list(range(n)))]
    for depth in range(max_levels + 1):
        nxt = []
        lvl = []
        for first, pkts, origin in work:
            c = dict(cfg, first=first)
            op = configs.oracle_parser(c)
            data, offs, caps = pack(pkts)
            ref = op.decode(data, offs, caps)
            pl = peel(c, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], kinds, gre_checksum)
            lvl.append(dict(first=first, packets=pkts, origin=origin, results=ref, peel=pl, data=data, offsets=offs,
                            caplens=caps))
            for i, g in enumerate(origin):
                rec = ref["records"][i]
                st = int(rec["status"])
                nl = (st >> 8) & 0xfff
                lst = (op.decoded_list(pkts[i]) if nl > 16 else
                       [CODE_TYPE[(int(rec["layers"]) >> (4 * k)) & 15] for k in range(nl)])
                decoded[g] += lst
                trunc[g] = trunc[g] or bool(st & 0x80)
                v = int(pl["verdict"][i])
                if v < 0:
                    error[g] = op.error_string(st & 0x7f, ref["err_args"][2 * i], ref["err_args"][2 * i + 1]) \
                        if st & 0x7f else ""
                    continue
                t = pl["tunnels"][v]
                trunc[g] = trunc[g] or bool(t["status"] & 1)
                if t["err"]:
                    error[g] = error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"]))
                    continue
                decoded[g].append(TYPE_OF_KIND[int(t["kind"])])
                typ = int(t["next_type"])
                if t["inner_len"] == 0:
                    error[g] = ""
                elif typ not in Tables(cfg).dispatch:
                    error[g] = "" if typ == 0 or cfg.get("ignore_unsupported") else op.error_string(1, typ)
            T = Tables(cfg)
            by_type = {}
            for j in range(int(pl["counts"][0])):
                t = pl["tunnels"][j]
                if t["err"] or t["inner_len"] == 0 or int(t["next_type"]) not in T.dispatch:
                    continue
                i = int(pl["index"][j])
                a = int(t["inner_off"])
                by_type.setdefault(int(t["next_type"]), ([], []))
                by_type[int(t["next_type"])][0].append(pkts[i][a:a + int(t["inner_len"])])
                by_type[int(t["next_type"])][1].append(origin[i])
            # class order: Ethernet, Dot1Q, IPv4, IPv6, then any other decodable type
            order = sorted(by_type, key=lambda lt: (CLASS_TYPE.index(lt) if lt in CLASS_TYPE else 9, lt))
            nxt += [(lt, by_type[lt][0], by_type[lt][1]) for lt in order]
        levels.append(lvl)
        work = nxt
        if not work:
            break
    else:
        raise RuntimeError("more than %d tunnel levels" % max_levels)
    return dict(decoded=decoded, error=error, truncated=trunc, levels=levels)
