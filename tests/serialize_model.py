"""Plain-Python restatement of include/gpk_serialize.h: the reference's
SerializeLayers (writer.go:207-218) over the layer list the header defines,
driven by one packet's source bytes, its gpk_layout and a gpk_fields record.

serialize_packet() -> (status, a0, a1, bytes); serialize_batch() packs the
results as gpk_serialize_batch does. The yardstick of tests/test_serialize_*.py.

Layer by layer:
  Ethernet  layers/ethernet.go:68-105     Dot1Q  layers/dot1q.go:61-76
  IPv4      layers/ip4.go:78-175          IPv6   layers/ip6.go:139-218
  HopByHop  layers/ip6.go:476-506, TLVs :314-325, :348-409, jumbo :53-134, :539-548
  TCP       layers/tcp.go:194-249         UDP    layers/udp.go:61-105
  pseudo-header  layers/tcpip.go:26-69    sum    checksum.go:35-58
"""
import numpy as np

ABSENT = 0xFFFFFFFF
M32 = 0xFFFFFFFF
ETH, D1Q, IP4, IP6, EXT, TCP, UDP, PAY = range(8)
SER_SLOTS = (ETH, D1Q, IP4, IP6, TCP, UDP)

OK = 0
# the reference's errors
ERR_ETH_TYPE_LENGTH = 1     # a0 = EthernetType, a1 = Length      ethernet.go:87
ERR_ETH_LENGTH = 2          # a0 = Length                         ethernet.go:89
ERR_IP6_FIT_LEN = 3         # a0 = payload length                 ip6.go:152
ERR_IP6_JUMBO_MISSING = 4   #                                     ip6.go:159
ERR_IP6_JUMBO_TLV_LEN = 5   #                                     ip6.go:68
ERR_IP6_JUMBO_SMALL = 6     #                                     ip6.go:72
ERR_IP6_JUMBO_TLV_SHORT = 7  # a0 = option length                 ip6.go:129
ERR_HBH_MULT8 = 8           #                                     ip6.go:494
ERR_IP6_FIT = 9             #                                     ip6.go:193
ERR_L4_NO_NETWORK = 10      #                                     tcpip.go:56
# scope decisions
ENOLAYER, EHBHLONG, EJUMBOADD, EINDEX, ELAYOUT = -40, -41, -42, -43, -44

ERROR_TEXT = {
    ERR_ETH_TYPE_LENGTH: "ethernet type %s not compatible with length value %d",
    ERR_ETH_LENGTH: "invalid ethernet length %d",
    ERR_IP6_FIT_LEN: "Cannot fit payload length of %d into IPv6 packet",
    ERR_IP6_JUMBO_MISSING: "Missing jumbo length hop-by-hop option",
    ERR_IP6_JUMBO_TLV_LEN: "Jumbo length TLV data must have length 4",
    ERR_IP6_JUMBO_SMALL: "Jumbo length cannot be less than 65536",
    ERR_IP6_JUMBO_TLV_SHORT: "Jumbo TLV too short (%d bytes)",
    ERR_HBH_MULT8: "IPv6HopByHop actual length must be multiple of 8",
    ERR_IP6_FIT: "Cannot fit payload into IPv6 header",
    ERR_L4_NO_NETWORK: "TCP/IP layer 4 checksum cannot be computed without network layer... call "
                       "SetNetworkLayerForChecksum to set which layer to use",
}


def compute_checksum(data, csum=0):
    """gopacket.ComputeChecksum, checksum.go:35-50: wraps mod 2^32."""
    a = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.uint64)
    csum += int(a[0::2].sum()) << 8
    csum += int(a[1::2].sum())
    return csum & M32


def fold_checksum(csum):
    """gopacket.FoldChecksum, checksum.go:53-58."""
    while csum > 0xFFFF:
        csum = (csum >> 16) + (csum & 0xFFFF)
    return ~csum & 0xFFFF


def _be16(v):
    return bytes(((v >> 8) & 0xFF, v & 0xFF))


def _bits(raw, nbits):
    v = int.from_bytes(bytes(bytearray(raw)), "little")
    return [k for k in range(nbits) if v >> k & 1]


class _Err(Exception):
    def __init__(self, status, a0=0, a1=0):
        self.args3 = (status, a0, a1)


def _src_jumbo_len(pkt, h, cap):
    """the value of the first jumbo option of the HopByHop header at h, walked as
    IPv6HopByHop.DecodeFromBytes walks it (ip6.go:509-526); None when there is none"""
    actual = pkt[h + 1] * 8 + 8
    off = 2
    while off < actual and h + off < cap:
        t = pkt[h + off]
        if t == 0:
            off += 1
            continue
        if h + off + 1 >= cap:
            break
        ln = pkt[h + off + 1]
        if t == 0xC2 and ln == 4 and h + off + 6 <= cap:
            return int.from_bytes(pkt[h + off + 2:h + off + 6], "big")
        off += 2 + ln
    return None


def _src_hdr(pkt, k, s, lim):
    """the source Contents length of slot k at s, or None when it leaves [s, lim)"""
    need = {ETH: 14, D1Q: 4, IP4: 20, IP6: 40, TCP: 20, UDP: 8}[k]
    if s + need > lim:
        return None
    if k == IP4:
        need = (pkt[s] & 15) * 4
    elif k == TCP:
        need = (pkt[s + 12] >> 4) * 4
    elif k == IP6 and pkt[s + 6] == 0:
        if s + 42 > lim:
            return None
        if pkt[s + 4] | pkt[s + 5]:  # inline HopByHop, not a jumbogram: ip6.go:239-263
            need = 40 + pkt[s + 41] * 8 + 8
    if need < {IP4: 20, TCP: 20}.get(k, 0) or s + need > lim:
        return None
    return need


def _tail_end(pkt, k, s, e):
    """the end of LayerPayload() of the innermost slot k, slice [s, e)"""
    if k == ETH:  # ethernet.go:49-61
        t = pkt[s + 12] << 8 | pkt[s + 13]
        return min(e, s + 14 + t) if t < 0x0600 else e
    if k == IP4:  # ip4.go:184-214
        ln = pkt[s + 2] << 8 | pkt[s + 3]
        if ln == 0:
            ln = (e - s) & 0xFFFF
        return min(e, s + ln)
    if k == IP6:  # ip6.go:239-275
        ln = pkt[s + 4] << 8 | pkt[s + 5]
        if pkt[s + 6] == 0:
            if ln == 0:
                j = _src_jumbo_len(pkt, s + 40, e)
                return min(e, s + 40 + (j or 0))
            return min(e, s + 40 + pkt[s + 41] * 8 + 8 + ln)
        return min(e, s + 40 + ln)
    if k == UDP:  # udp.go:44-55
        ln = pkt[s + 4] << 8 | pkt[s + 5]
        return min(e, s + ln) if ln >= 8 else e
    return e  # Dot1Q, TCP


def _options(pkt, s, raw_map, cap):
    """the IPv4 / TCP option list of the header at s from its option map: [(type, start, length)]"""
    out = []
    for k in _bits(raw_map, 40):
        b = s + 20 + k
        if b >= cap:
            raise _Err(ELAYOUT)
        t = pkt[b]
        if t in (0, 1):
            ln = 1
        else:
            if b + 1 >= cap:
                raise _Err(ELAYOUT)
            ln = pkt[b + 1]
            if ln < 2 or b + ln > cap:
                raise _Err(ELAYOUT)
        out.append((t, b, ln))
    return out


def _ip4_header(pkt, s, f, fix, csum, after, cap):
    """IPv4.SerializeTo, ip4.go:78-169. after = len(b.Bytes()) before the call."""
    opts = _options(pkt, s, f["ip4_opt_map"], cap)
    body = b"".join(pkt[b:b + ln] for (_, b, ln) in opts)  # type 0 / 1: the byte itself; else type, length, data
    size = len(body) + (-len(body) % 4)  # getIPv4OptionSize; Padding is never written
    ihl, length = int(f["ip4_ihl"]), int(f["ip4_length"])
    if fix:
        ihl = 5 + size // 4
        length = (20 + size + after) & 0xFFFF
    h = bytearray(20 + size)
    h[0] = (int(f["ip4_version"]) << 4 | ihl) & 0xFF
    h[1] = int(f["ip4_tos"])
    h[2:4] = _be16(length)
    h[4:6] = _be16(int(f["ip4_id"]))
    h[6:8] = _be16(int(f["ip4_flags_frag"]))
    h[8] = int(f["ip4_ttl"])
    h[9] = int(f["ip4_protocol"])
    h[12:16] = bytes(bytearray(f["ip4_src"]))
    h[16:20] = bytes(bytearray(f["ip4_dst"]))
    h[20:20 + len(body)] = body
    ck = int(f["ip4_checksum"])
    if csum:
        ck = fold_checksum(compute_checksum(h))
    h[10:12] = _be16(ck)
    return bytes(h)


def _tcp_header_size(pkt, s, f, fix, cap):
    opts = _options(pkt, s, f["tcp_opt_map"], cap)
    optlen = sum(1 if t in (0, 1) else 2 if t == 30 else ln for (t, _, ln) in opts)
    pad = b""
    if opts and opts[-1][0] == 0:  # tcp.go:341-344: the source's bytes after End of options
        hend = s + (pkt[s + 12] >> 4) * 4
        pad = pkt[opts[-1][1] + 1:hend]
    if fix and optlen % 4:
        pad = bytes(4 - optlen % 4)
    if optlen + len(pad) > 40:  # options that overlap: not a map the decode wrote
        raise _Err(ELAYOUT)
    return opts, optlen, pad


def _tcp_header(pkt, s, f, fix, cap):
    """TCP.SerializeTo without the checksum, tcp.go:194-236"""
    opts, optlen, pad = _tcp_header_size(pkt, s, f, fix, cap)
    doff = int(f["tcp_data_offset"])
    if fix:
        doff = ((len(pad) + optlen + 20) // 4) & 0xFF
    h = bytearray(20 + optlen + len(pad))
    h[0:2] = _be16(int(f["tcp_src_port"]))
    h[2:4] = _be16(int(f["tcp_dst_port"]))
    h[4:8] = int(f["tcp_seq"]).to_bytes(4, "big")
    h[8:12] = int(f["tcp_ack"]).to_bytes(4, "big")
    h[12:14] = _be16((doff << 12 | int(f["tcp_flags"]) & 0x1FF) & 0xFFFF)
    h[14:16] = _be16(int(f["tcp_window"]))
    h[18:20] = _be16(int(f["tcp_urgent"]))
    at = 20
    for (t, b, ln) in opts:
        if t in (0, 1):
            h[at] = t
            at += 1
        elif t == 30:  # MPTCP decodes with no OptionData: tcp.go:347-533
            h[at] = 30
            h[at + 1] = 2 if fix else ln
            at += 2
        else:
            h[at:at + ln] = pkt[b:b + ln]
            at += ln
    h[at:] = pad
    return h


def _hbh_options(pkt, h, raw_map, cap):
    out = []
    for k in _bits(raw_map, 24):
        b = h + 2 + k
        if b >= cap:
            raise _Err(ELAYOUT)
        t = pkt[b]
        if t == 0:
            out.append((0, b"\0\0"))  # Pad1 decodes to {0, OptionLength 0}: ip6.go:314-325 writes two bytes
            continue
        if b + 1 >= cap or b + 2 + pkt[b + 1] > cap:
            raise _Err(ELAYOUT)
        out.append((t, pkt[b:b + 2 + pkt[b + 1]]))
    return out


def _tlv_padding(n):  # serializeTLVOptionPadding, ip6.go:348-365
    return b"" if n <= 0 else b"\0" if n == 1 else bytes((1, n - 2)) + bytes(n - 2)


def _hbh_header(pkt, h, f, fix, jumbo, cap):
    """IPv6HopByHop.SerializeTo, ip6.go:476-506, after addIPv6JumboOption when fix and jumbo"""
    if pkt[h + 1] > 2:
        raise _Err(EHBHLONG)
    opts = _hbh_options(pkt, h, f["hbh_opt_map"], cap)
    jpos = None
    out = bytearray(2)
    seen = False
    for (t, raw) in opts:
        if fix and jumbo and t == 0xC2 and not seen:  # SetJumboLength: ip6.go:539-548, alignment 4n+2
            seen = True
            if len(raw) < 6:
                raise _Err(EJUMBOADD)  # the reference panics
            if len(out) % 4 != 2:  # ip6.go:374-390: the reference would insert a padding option
                raise _Err(EJUMBOADD)
            jpos = len(out)
            raw = raw[:2] + bytes(4) + raw[6:]
        out += raw
    if fix and jumbo and not seen:
        raise _Err(EJUMBOADD)
    if fix:
        out += _tlv_padding(len(out) % 8)  # ip6.go:399-407
    if len(out) % 8:
        raise _Err(ERR_HBH_MULT8)
    out[0] = pkt[h]
    out[1] = (len(out) // 8 - 1) & 0xFF if fix else pkt[h + 1]
    return out, jpos


def _ip6_header(pkt, s, f, fix, after, cap):
    """IPv6.SerializeTo, ip6.go:139-218"""
    has_hbh = pkt[s + 6] == 0
    plen = after
    jumbo = plen > 65535
    hbh = bytearray()
    if jumbo and not fix:
        if not has_hbh:
            raise _Err(ERR_IP6_FIT_LEN, plen)
        if pkt[s + 41] > 2:
            raise _Err(EHBHLONG)
        first = [raw for (t, raw) in _hbh_options(pkt, s + 40, f["hbh_opt_map"], cap) if t == 0xC2][:1]
        if not first:
            raise _Err(ERR_IP6_JUMBO_MISSING)
        if len(first[0]) != 6:
            raise _Err(ERR_IP6_JUMBO_TLV_LEN)
        if int.from_bytes(first[0][2:6], "big") <= 65535:
            raise _Err(ERR_IP6_JUMBO_SMALL)
    if jumbo and fix and not has_hbh:
        raise _Err(EJUMBOADD)
    nh = int(f["ip6_next_header"])
    if has_hbh:
        nh = 0  # ip6.go:173-177
        hbh, jpos = _hbh_header(pkt, s + 40, f, fix, jumbo, cap)
        plen += len(hbh)
        if fix and jumbo:  # setIPv6PayloadJumboLength, ip6.go:105-134
            ln = hbh[jpos + 1]
            if ln != 4:
                raise _Err(ERR_IP6_JUMBO_TLV_SHORT, ln)
            hbh[jpos + 2:jpos + 6] = (plen & M32).to_bytes(4, "big")
    if not jumbo and plen > 65535:
        raise _Err(ERR_IP6_FIT)
    length = int(f["ip6_length"])
    if fix:
        length = 0 if jumbo else plen & 0xFFFF
    tc, fl = int(f["ip6_traffic_class"]), int(f["ip6_flow_label"])
    h = bytearray(40)
    h[0] = (int(f["ip6_version"]) << 4 | tc >> 4) & 0xFF
    h[1] = (tc << 4 | (fl >> 16) & 0xFF) & 0xFF
    h[2:4] = _be16(fl & 0xFFFF)
    h[4:6] = _be16(length)
    h[6] = nh
    h[7] = int(f["ip6_hop_limit"])
    h[8:24] = bytes(bytearray(f["ip6_src"]))
    h[24:40] = bytes(bytearray(f["ip6_dst"]))
    return bytes(h + hbh)


def _check_lists(pkt, k, s, f, fix, cap):
    """ELAYOUT for an option map that does not describe this packet, before any layer is written"""
    if k == IP4 and sum(ln for (_, _, ln) in _options(pkt, s, f["ip4_opt_map"], cap)) > 40:
        raise _Err(ELAYOUT)
    if k == TCP:
        _tcp_header_size(pkt, s, f, fix, cap)
    if k == IP6 and pkt[s + 6] == 0 and pkt[s + 41] <= 2:
        if sum(len(raw) for (_, raw) in _hbh_options(pkt, s + 40, f["hbh_opt_map"], cap)) > 2000:
            raise _Err(ELAYOUT)


def serialize_packet(pkt, start, end, f, fix, csum):
    """-> (status, a0, a1, bytes). pkt: the source packet; start, end: its gpk_layout; f: a gpk_fields record."""
    pkt = bytes(pkt)
    cap = len(pkt)
    try:
        return (OK, 0, 0, _serialize(pkt, cap, [int(x) for x in start], [int(x) for x in end], f, bool(fix), bool(csum)))
    except _Err as e:
        return e.args3 + (b"",)


def _serialize(pkt, cap, start, end, f, fix, csum):
    present = int(f["present"])
    for k in SER_SLOTS:
        if present >> k & 1 and start[k] == ABSENT:
            raise _Err(ENOLAYER)
    slots = sorted((start[k], k) for k in SER_SLOTS if start[k] != ABSENT)
    # the layer list: ("gap", bytes) and (k, source start)
    layers = []
    prev = 0
    inner = None
    for (s, k) in slots:
        lim = min(end[k], cap)
        hdr = _src_hdr(pkt, k, s, lim) if s >= prev else None
        if hdr is None or (inner is not None and inner[0] in (TCP, UDP)):
            raise _Err(ELAYOUT)  # not this packet's layout, or a transport slice that is not the innermost
        if s > prev:
            layers.append(("gap", pkt[prev:s]))
        if present >> k & 1:
            _check_lists(pkt, k, s, f, fix, cap)
            layers.append((k, s))
        prev = s + hdr
        inner = (k, s, lim)
    tail_end = _tail_end(pkt, inner[0], inner[1], inner[2]) if inner else cap
    if tail_end > prev:
        layers.append(("gap", pkt[prev:tail_end]))
    nets = [(s, k) for (k, s) in layers if k in (IP4, IP6)]
    net = max(nets)[1] if nets else None  # the pseudo-header: the serialized network layer with the greatest start
    buf = b""
    for (k, s) in reversed(layers):  # writer.go:207-218: innermost first
        if k == "gap":
            buf = s + buf  # gopacket.Payload.SerializeTo
        elif k == TCP or k == UDP:
            if k == TCP:
                h = _tcp_header(pkt, s, f, fix, cap)
                ckat, ck, proto = 16, int(f["tcp_checksum"]), 6
            else:  # udp.go:61-105
                jumbo = net == IP6 and len(buf) + 8 > 65535
                length = int(f["udp_length"])
                if fix:
                    length = 0 if jumbo else (len(buf) + 8) & 0xFFFF
                h = bytearray(_be16(int(f["udp_src_port"])) + _be16(int(f["udp_dst_port"])) + _be16(length) + b"\0\0")
                ckat, ck, proto = 6, int(f["udp_checksum"]), 17
            if csum:
                if net is None:
                    raise _Err(ERR_L4_NO_NETWORK)
                addrs = bytes(bytearray(f["ip4_src"])) + bytes(bytearray(f["ip4_dst"])) if net == IP4 else \
                    bytes(bytearray(f["ip6_src"])) + bytes(bytearray(f["ip6_dst"]))
                n = len(h) + len(buf)
                c = (compute_checksum(addrs) + proto + (n & 0xFFFF) + (n >> 16)) & M32  # tcpip.go:58-65
                ck = fold_checksum(compute_checksum(bytes(h) + buf, c))
                if k == UDP and ck == 0:
                    ck = 0xFFFF
            h[ckat:ckat + 2] = _be16(ck)
            buf = bytes(h) + buf
        elif k == IP4:
            buf = _ip4_header(pkt, s, f, fix, csum, len(buf), cap) + buf
        elif k == IP6:
            buf = _ip6_header(pkt, s, f, fix, len(buf), cap) + buf
        elif k == D1Q:
            buf = _be16(int(f["d1q_tci"])) + _be16(int(f["d1q_type"])) + buf
        elif k == ETH:
            et, ln = int(f["eth_type"]), int(f["eth_length"])
            if ln != 0 or et == 0:
                if fix:
                    ln = len(buf) & 0xFFFF
                if et != 0:
                    raise _Err(ERR_ETH_TYPE_LENGTH, et, ln)
                if ln > 0x0600:
                    raise _Err(ERR_ETH_LENGTH, ln)
                et = ln
            buf = bytes(bytearray(f["eth_dst"])) + bytes(bytearray(f["eth_src"])) + _be16(et) + buf
            if len(buf) < 60:
                buf += bytes(60 - len(buf))
    return buf


def serialize_batch(data, offsets, caplens, layouts, fields, order, fix, csum, out_cap=None):
    """What gpk_serialize_batch leaves: dict(out, offsets[m+1], caplens[m], status[m], err_args[2m], counts[4]).
    out holds counts[1] bytes; a packet that does not end inside out_cap is left as zeros there."""
    n = len(caplens)
    idx = range(n) if order is None else [int(x) for x in order]
    m = len(idx)
    offs = np.zeros(m + 1, np.uint64)
    lens = np.zeros(m, np.uint32)
    status = np.zeros(m, np.int32)
    args = np.zeros(2 * m, np.uint32)
    parts, at, wrote, errors = [], 0, 0, 0
    data = bytes(bytearray(data))
    for j, i in enumerate(idx):
        if i >= n:
            st, a0, a1, b = EINDEX, 0, 0, b""
        else:
            o, c = int(offsets[i]), int(caplens[i])
            st, a0, a1, b = serialize_packet(data[o:o + c], layouts[i]["start"], layouts[i]["end"], fields[i], fix, csum)
        status[j], args[2 * j], args[2 * j + 1], lens[j] = st, a0, a1, len(b)
        errors += st != OK
        fits = out_cap is None or at + len(b) <= out_cap
        wrote += st == OK and fits
        parts.append(b if fits else bytes(len(b)))
        at += len(b)
        offs[j + 1] = at
    cap = at if out_cap is None else out_cap
    return dict(out=np.frombuffer(b"".join(parts), np.uint8), offsets=offs, caplens=lens, status=status, err_args=args,
                counts=np.array([wrote, at, errors, at > cap], np.uint64), fits=[int(offs[j + 1]) <= cap for j in range(m)])


def error_text(status, a0, a1, ethertype_name=lambda v: str(v)):
    """the reference's error text of a positive status"""
    t = ERROR_TEXT[status]
    if status == ERR_ETH_TYPE_LENGTH:
        return t % (ethertype_name(a0), a1)
    return t % a0 if "%d" in t else t
