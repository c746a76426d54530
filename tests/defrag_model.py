"""Pure-Python restatement of ip4defrag's reassembly (ip4defrag/defrag.go):
fragmentList.insert (:214-271), build (:276-326) and the tail of
DefragIPv4WithTimestamp (:113-132), quirks included, in uint16 arithmetic
where Go uses uint16. TEST INFRASTRUCTURE ONLY: the checker of
gopacket_amd/csrc/gpk_defrag.hip (include/gpk_defrag.h).

Input: the packets, the decode oracle's records and layouts, and
oracle/flows_oracle.py's keying (dontDefrag and securityChecks, :86-94). One
run behaves like a fresh NewIPv4Defragmenter() fed the packets in order.

  - fragOffset >= Highest pushes back; otherwise an equal FragOffset is
    ignored (nil, nil) before any counter moves, else the fragment goes before
    the first larger offset; with no larger offset it is NOT listed but the
    counters still move
  - fragLength = Length - 20 whatever the IHL; Payload is the decode's
    data[IHL*4 : min(len(data), Length)]
  - build: the overlap branch adds frag.FragOffset*8 to currentOffset;
    "invalid fragment", "hole found"; frag.Payload[startAt:] past the payload
    panics in Go -> EPANIC; a failed build leaves the list as it was
  - out == nil && List.Len()+1 > 8192 flushes the key: EMAXLEN (checked after
    every nil result, EPANIC included)
  - out: Length = Highest, every other field from `in`, the completing packet

Harness rule: "the IPv4" of a packet is its layout slot's last IPv4, the one
the grouping keyed. Timeouts (DiscardOlderThan, LastSeen) are not modelled.
"""
from oracle import flows_oracle as FO

HELD, EHOLE, EINVALID, EMAXLEN, EPANIC = -16, -17, -18, -19, -20
MAX_LIST = 8192
SLOT_IP4 = FO.SLOT_IP4


class Frag:
    __slots__ = ("idx", "fo", "length", "mf", "ihl", "start", "payload")

    def __init__(self, idx, pkt, lay):
        s, e = int(lay["start"][SLOT_IP4]), int(lay["end"][SLOT_IP4])
        data = pkt[s:e]
        length = data[2] << 8 | data[3]
        if length == 0:
            length = len(data) & 0xFFFF
        ff = data[6] << 8 | data[7]
        self.idx, self.fo, self.length, self.mf = idx, ff & 0x1FFF, length, (ff >> 13) & 1
        self.ihl, self.start = data[0] & 15, s
        self.payload = bytes(data[self.ihl * 4:min(len(data), length)])


class FragList:
    def __init__(self):
        self.list, self.highest, self.current, self.final, self.counted = [], 0, 0, False, []

    def insert(self, f):
        """-> (payload bytes or None, verdict)"""
        off = f.fo * 8
        if off >= self.highest:
            self.list.append(f)
        else:
            for k, e in enumerate(self.list):
                if f.fo == e.fo:
                    return None, HELD
                if f.fo < e.fo:
                    self.list.insert(k, f)
                    break
        frag_len = (f.length - 20) & 0xFFFF
        if self.highest < (off + frag_len) & 0xFFFF:
            self.highest = (off + frag_len) & 0xFFFF
        self.current = (self.current + frag_len) & 0xFFFF
        self.counted.append(f.idx)
        if not f.mf:
            self.final = True
        if self.final and self.highest == self.current:
            return self.build()
        return None, HELD

    def build(self):
        final, cur = [], 0
        for e in self.list:
            eo = e.fo * 8
            if eo == cur:
                final.append(e.payload)
                cur = (cur + e.length - 20) & 0xFFFF
            elif eo < cur:
                start_at = cur - eo
                if start_at > (e.length - 20) & 0xFFFF:
                    return None, EINVALID
                if start_at > len(e.payload):
                    return None, EPANIC
                final.append(e.payload[start_at:])
                cur = (cur + eo) & 0xFFFF
            else:
                return None, EHOLE
        return b"".join(final), 0


def csum(b):
    s = 0
    for k in range(0, len(b), 2):
        s += b[k] << 8 | b[k + 1]
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def datagram_bytes(pkt, f, payload):
    """`in` from the packet start through its IPv4 header with Flags/FragOffset
    0, Total Length = header + payload (0 past 16 bits) and a fresh checksum,
    then the payload (include/gpk_defrag.h)."""
    s, hl = f.start, f.ihl * 4
    h = bytearray(pkt[:s + hl])
    tot = hl + len(payload)
    if tot > 0xFFFF:
        tot = 0
    h[s + 2:s + 4] = tot.to_bytes(2, "big")
    h[s + 6:s + 8] = b"\x00\x00"
    h[s + 10:s + 12] = b"\x00\x00"
    h[s + 10:s + 12] = csum(h[s:s + hl]).to_bytes(2, "big")
    return bytes(h) + payload


def run(packets, records, layouts):
    """-> dict(verdict: per packet (>= 0: the datagram it completed),
    datagrams: [dict(last, length, payload, payload_off, data)] in completion order,
    pending: ascending packet indices still counted in an unflushed key,
    pending_by_key: key -> those indices)."""
    flows, verdict, datagrams = {}, [], []
    for i, pkt in enumerate(packets):
        k = FO.packet_key(FO.DEFRAG, pkt, records[i], layouts[i], 0, 8)
        if isinstance(k, int):
            verdict.append(k)
            continue
        f = Frag(i, pkt, layouts[i])
        fl = flows.setdefault(k, FragList())
        out, v = fl.insert(f)
        if out is None and len(fl.list) + 1 > MAX_LIST:
            del flows[k]
            v = EMAXLEN
        if out is not None:
            v = len(datagrams)
            datagrams.append(dict(last=i, length=fl.highest, payload=out, payload_off=f.start + f.ihl * 4,
                                  data=datagram_bytes(pkt, f, out)))
            del flows[k]
        verdict.append(v)
    by_key = {k: list(fl.counted) for k, fl in flows.items()}
    return dict(verdict=verdict, datagrams=datagrams, pending=sorted(i for v in by_key.values() for i in v),
                pending_by_key=by_key, lists={k: [e.idx for e in fl.list] for k, fl in flows.items()},
                state={k: (fl.highest, fl.current, fl.final) for k, fl in flows.items()})
