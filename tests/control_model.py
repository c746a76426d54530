"""Executable statement of the control-layer rules (include/gpk_control.h,
DESIGN.md §21), independent of the C++ in gopacket_amd/csrc/gpk_control_rules.h.

  decode_icmp4 / decode_icmp6 / decode_echo / decode_arp
                        layers/icmp4.go:221-232, icmp6.go:189-198,
                        icmp6msg.go:155-164, arp.go:42-67 on a Go-style slice
  icmp6_next            ICMPv6.NextLayerType, icmp6.go:230-261
  verify4 / verify6     VerifyChecksum, icmp4.go:265-276, icmp6.go:263-277 with
                        computeChecksum of tcpip.go:54-69
  control_packet        candidate rule, first layer, the rest of the loop
                        (layers_decoder.go:60-79)
  control(cfg, ...)     gpk_control_batch's outputs
  compose(cfg, packets) DecodeLayers with the four layers (and, optionally, the
                        tunnel layers) added to the parser of `cfg`

The candidate's payload and next type come from tunnel_model.last_payload, and
the six-layer decode of every level is the oracle's (oracle/).
"""
import numpy as np

import tunnel_model as TM
from tunnel_model import Sl, Tables, compute_checksum, fold  # noqa: F401
from gopacket_amd import _lib

LT_PAYLOAD, LT_ARP, LT_ICMPV4, LT_ICMPV6, LT_ECHO = 2, 10, 19, 57, 132
KIND_OF_TYPE = {LT_ICMPV4: 1, LT_ICMPV6: 2, LT_ECHO: 4, LT_ARP: 8}
ICMP6_NEXT = {128: 132, 129: 132, 133: 124, 134: 125, 135: 126, 136: 127, 137: 128, 132: 136, 131: 135, 143: 138}
NO_NETWORK = ("TCP/IP layer 4 checksum cannot be computed without network layer... call "
              "SetNetworkLayerForChecksum to set which layer to use")


class GoError(Exception):
    def __init__(self, code, a0=0, a1=0):
        Exception.__init__(self, code, a0, a1)
        self.code, self.a0, self.a1 = code, a0, a1


def error_text(code, a0=0, a1=0):
    return {0: "", 80: "ICMP layer less then 8 bytes for ICMPv4 packet",
            81: "ICMP layer less then 4 bytes for ICMPv6 packet", 82: "ICMP layer less then 4 bytes for ICMPv6 Echo",
            83: "ARP length %d too short" % a0, 84: "ARP length %d too short, %d expected" % (a0, a1)}[code]


def decode_icmp4(d):
    if d.len < 8:
        raise GoError(80)
    return dict(kind=1, typecode=d[0] << 8 | d[1], checksum=d.be16(2), id=d.be16(4), seq=d.be16(6),
                contents=d.sl(0, 8), payload=d.sl(8), next_type=LT_PAYLOAD)


def icmp6_next(typ, payload_len):
    if typ == 130:
        return 139 if payload_len > 20 else 137
    return ICMP6_NEXT.get(typ, LT_PAYLOAD)


def decode_icmp6(d):
    if d.len < 4:
        raise GoError(81)
    payload = d.sl(4)
    return dict(kind=2, typecode=d[0] << 8 | d[1], checksum=d.be16(2), contents=d.sl(0, 4), payload=payload,
                next_type=icmp6_next(d[0], payload.len))


def decode_echo(d):
    """No BaseLayer is set: Contents and Payload are empty."""
    if d.len < 4:
        raise GoError(82)
    return dict(kind=4, id=d.be16(0), seq=d.be16(2), contents=d.sl(0, 0), payload=d.sl(0, 0), next_type=LT_PAYLOAD)


def decode_arp(d):
    if d.len < 8:
        raise GoError(83, d.len)
    hw, prot = d[4], d[5]
    n = 8 + 2 * hw + 2 * prot
    if d.len < n:
        raise GoError(84, d.len, n)
    return dict(kind=8, arp_addr_type=d.be16(0), arp_protocol=d.be16(2), arp_hw_size=hw, arp_prot_size=prot,
                arp_operation=d.be16(6), contents=d.sl(0, n), payload=d.sl(n), next_type=LT_PAYLOAD,
                addresses=(d.sl(8, 8 + hw).bytes(), d.sl(8 + hw, 8 + hw + prot).bytes(),
                           d.sl(8 + hw + prot, 8 + 2 * hw + prot).bytes(), d.sl(8 + 2 * hw + prot, n).bytes()))


DECODERS = {1: decode_icmp4, 2: decode_icmp6, 4: decode_echo, 8: decode_arp}
TYPE_OF_KIND = {1: LT_ICMPV4, 2: LT_ICMPV6, 4: LT_ECHO, 8: LT_ARP}


def verify4(message, existing):
    """(Valid, Correct, Actual) of ICMPv4.VerifyChecksum."""
    correct = fold((compute_checksum(message) - existing) & 0xffffffff)
    return correct == existing, correct, existing


def sum_init(addresses, length):
    """computeChecksum's start value: the address words, the protocol (58) and the length."""
    s = 0
    for i in range(0, len(addresses), 2):
        s += addresses[i] << 8 | addresses[i + 1]
    return (s + 58 + (length & 0xffff) + (length >> 16)) & 0xffffffff


def verify6(message, existing, addresses):
    """(Valid, Correct, Actual) of ICMPv6.VerifyChecksum; addresses: SrcIP‖DstIP
    of the pseudo-header's network layer."""
    total = (compute_checksum(message) + sum_init(addresses, len(message))) & 0xffffffff
    correct = fold((total - existing) & 0xffffffff)
    return correct == existing, correct, existing


def network_addresses(pkt, rec, lay):
    """SrcIP‖DstIP of the last network layer of the decoded list, or None."""
    nl = (int(rec["status"]) >> 8) & 0xfff
    for k in reversed(range(nl)):
        code = (int(rec["layers"]) >> (4 * k)) & 15
        if code in (3, 4):
            s = int(lay["start"][code - 1])
            if s == 0xffffffff:
                return None
            return pkt[s + 12:s + 20] if code == 3 else pkt[s + 8:s + 40]
    return None


def control_packet(T, pkt, rec, lay, err_a0, kinds, checksum):
    """One packet: (class or CTL_NONE / CTL_UNKNOWN, record dict or None)."""
    status = int(rec["status"])
    nl = (status >> 8) & 0xfff
    if nl > 16:
        return _lib.CTL_UNKNOWN, None
    err = status & 0x7f
    if nl == 0 or err not in (0, 1):
        return _lib.CTL_NONE, None
    dec = TM.CODE_DEC[(int(rec["layers"]) >> (4 * (nl - 1))) & 15]
    if dec in ("PAYLOAD", "FRAGMENT"):
        return _lib.CTL_NONE, None
    k = TM.SLOTS.index(dec)
    off, ln, nxt = TM.last_payload(T, dec, pkt, int(lay["start"][k]), int(lay["end"][k]))
    if err == 1:  # UnsupportedLayerType names the next type: a second derivation of it
        assert nxt == err_a0, (nxt, err_a0)
    kind = KIND_OF_TYPE.get(nxt, 0) & kinds
    if not kind or ln == 0:
        return _lib.CTL_NONE, None
    d = Sl(pkt, off, ln, len(pkt) - off)
    t = dict(kind=kind, hdr_off=off)
    try:
        r = DECODERS[kind](d)
    except GoError as e:
        t.update(err=e.code, err_a0=e.a0, err_a1=e.a1, status=1)
        return _lib.CTL_CLASS_FAILED, t
    contents, payload = r.pop("contents"), r.pop("payload")
    t.update(r)
    t.pop("addresses", None)
    t.update(contents_len=contents.len, payload_len=payload.len,
             payload_off=payload.off, status=0)
    lts = [TYPE_OF_KIND[kind]]
    # the loop goes on: layers_decoder.go:60-79
    nxt = r["next_type"]
    if payload.len:
        if nxt == LT_ECHO and kinds & 4:
            try:
                e = decode_echo(payload)
                t.update(id=e["id"], seq=e["seq"])
                lts.append(LT_ECHO)
            except GoError as ex:
                t.update(err=ex.code, status=1)
        elif nxt == LT_PAYLOAD and T.dispatch.get(LT_PAYLOAD) == "PAYLOAD":
            lts.append(LT_PAYLOAD)
        else:
            t["unsupported"] = nxt
    t["nlayers"] = len(lts)
    t["layer_types"] = lts + [0] * (3 - len(lts))
    if checksum and kind in (1, 2):
        msg = contents.bytes() + payload.bytes()
        if kind == 1:
            valid, correct, _ = verify4(msg, t["checksum"])
        else:
            adr = network_addresses(pkt, rec, lay)
            if adr is None:
                t["status"] |= 8
                valid = None
            else:
                t["sum_init"] = sum_init(adr, len(msg))
                valid, correct, _ = verify6(msg, t["checksum"], adr)
        if valid is not None:
            t["correct"] = correct
            t["status"] |= 2 | (4 if valid else 0)
    cls = {1: _lib.CTL_CLASS_ICMP4, 2: _lib.CTL_CLASS_ICMP6, 4: _lib.CTL_CLASS_ICMP6, 8: _lib.CTL_CLASS_ARP}[kind]
    return cls, t


def control(cfg, data, offsets, caplens, records, layouts, err_args=None, kinds=15, checksum=True, fill=0):
    """gpk_control_batch's outputs (arrays start as `fill` bytes)."""
    T = Tables(cfg)
    n = len(caplens)
    raw = bytes(np.ascontiguousarray(data, np.uint8))
    res = []
    for i in range(n):
        o, c = int(offsets[i]), int(caplens[i])
        a0 = int(err_args[2 * i]) if err_args is not None else None
        if a0 is not None and a0 >= 1 << 31:
            a0 -= 1 << 32
        res.append(control_packet(T, raw[o:o + c], records[i], layouts[i], a0, kinds, checksum))

    def arr(count, dt):
        a = np.empty(count, dt)
        a.view(np.uint8)[:] = fill
        return a
    out = dict(verdict=arr(n, np.int32), class_start=arr(5, np.uint32), index=arr(n, np.uint32),
               records=arr(n, _lib.CONTROL_DTYPE), counts=arr(8, np.uint32))
    j = sums = 0
    for c in range(_lib.CTL_NCLASS):
        out["class_start"][c] = j
        for i, (cls, t) in enumerate(res):
            if cls != c:
                continue
            out["verdict"][i] = j
            out["index"][j] = i
            rec = np.zeros(1, _lib.CONTROL_DTYPE)
            for name in _lib.CONTROL_DTYPE.names:
                if name in t:
                    rec[name] = t[name]
            out["records"][j] = rec[0]
            sums += bool(t.get("status", 0) & 2)
            j += 1
    out["class_start"][4] = j
    for i, (cls, t) in enumerate(res):
        if cls < 0:
            out["verdict"][i] = cls
    out["counts"][:] = 0
    out["counts"][0] = j
    out["counts"][1:5] = np.diff(out["class_start"].astype(np.int64))
    out["counts"][5] = sums
    return out


def compose(cfg, packets, kinds=15, checksum=True, tunnel_kinds=0):
    """DecodeLayers of every packet with the control layers `kinds` (and the
    tunnel layers `tunnel_kinds`) added to the parser of `cfg`: tunnel_model's
    composition, then the control pass over every level's part. A control
    candidate's last layer leads to a control type, so it is no tunnel
    candidate: the part is the packet's innermost. Returns tunnel_model.compose's
    dict; every level entry gains "control"."""
    import configs
    r = TM.compose(cfg, packets, kinds=tunnel_kinds)
    for lvl in r["levels"]:
        for part in lvl:
            c = dict(cfg, first=part["first"])
            ref = part["results"]
            ctl = control(c, part["data"], part["offsets"], part["caplens"], ref["records"], ref["layouts"],
                          ref["err_args"], kinds, checksum)
            part["control"] = ctl
            op = configs.oracle_parser(c)
            for i, g in enumerate(part["origin"]):
                v = int(ctl["verdict"][i])
                if v < 0:
                    continue
                t = ctl["records"][v]
                r["decoded"][g] += [int(x) for x in t["layer_types"][:int(t["nlayers"])]]
                r["truncated"][g] = r["truncated"][g] or bool(t["status"] & 1)
                if t["err"]:
                    r["error"][g] = error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"]))
                elif t["unsupported"] and not cfg.get("ignore_unsupported"):
                    r["error"][g] = op.error_string(1, int(t["unsupported"]))
                else:
                    r["error"][g] = ""
    return r
