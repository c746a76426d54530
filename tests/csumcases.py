"""Frames and batches that push the checksum sums to their ends: saturated
payloads and headers, the points where a 32-bit sum wraps, the residues the
fold maps to 0x0000 / 0xFFFF, and the lengths at which phase B of the decode
kernels changes path (gpk_kernels.hip dense_region, l_to_words).

Everything the tests expect comes from here and from the CPU oracle:
py_checksums is a second, independent statement of the reference's arithmetic
(checksum.go:35-58, tcpip.go:54-69, ip4.go:323-332, udp.go:144-158) in Python
integers and shares no code with oracle/; wave_plan restates dense_region's
predicate and is used only to assert that a case is what it claims to be.
"""
import collections
import functools
import struct

import numpy as np

M32 = 0xFFFFFFFF
ABSENT = 0xFFFFFFFF
ETH, D1Q, IP4, IP6, EXT, TCP, UDP, PAY = range(8)  # gpk_layout slots (include/gpk.h)
WAVE = 64


# ---- frames ---------------------------------------------------------------------

class Frame(bytes):
    """A packet's bytes and where its layers lie: l3 / l4 (offsets of the network
    header and of the bytes the transport decoder is handed), seg_end (end of the
    summed segment), field / ip4_field (offsets of the TCP/UDP and the IPv4
    checksum fields; None without one), payload (offset of the first payload
    byte), net ("ip4" / "ip6"), kind ("tcp" / "udp"), tags (802.1Q tags)."""

    def __new__(cls, data, **where):
        f = bytes.__new__(cls, data)
        f.__dict__.update(where)
        return f

    def replace(self, data):
        assert len(data) == len(self)
        return Frame(bytes(data), **self.__dict__)

    def segment(self):
        """The summed L4 segment as (start, end) inside the packet."""
        return self.l4, self.seg_end

    def layout(self):
        """The layer slices DecodeLayers hands the decoders (start, end per
        gpk_layout slot), from the builder's own arithmetic."""
        start, end = [ABSENT] * 8, [ABSENT] * 8
        n = len(self)

        def put(slot, s, e):
            start[slot], end[slot] = s, e
        if self.link == "eth":
            put(ETH, 0, n)
            if self.tags:
                put(D1Q, 14 + 4 * (self.tags - 1), n)  # the last tag decoded (last writer)
        put(IP4 if self.net == "ip4" else IP6, self.l3, n)
        put(TCP if self.kind == "tcp" else UDP, self.l4, self.seg_end)
        if self.seg_end > self.payload:
            put(PAY, self.payload, self.seg_end)
        return dict(start=start, end=end)


def _link(link, ethertype, tags, saturate):
    if link is None:
        return b""
    assert link == "eth"
    mac = b"\xff" * 12 if saturate else b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02"
    out = mac
    for tci in tags:
        out += struct.pack(">HH", 0x8100, tci)
    return out + struct.pack(">H", ethertype)


def frame(net, kind, payload=b"", link="eth", vlan=None, options=b"", saturate=False, field=0, ip4_field=0):
    """Ethernet (link="eth"; None: the bare network packet) + optional 802.1Q
    tags (vlan: one TCI or a list of them) / IPv4 (options: up to 40 bytes, a
    multiple of 4) or IPv6 / TCP or UDP / payload. saturate: every header field
    that may legally be all-ones is: MACs, tag TCIs, TOS, id, TTL, the reserved
    and DF flag bits (MF and the fragment offset stay 0: a fragment has no
    transport layer), traffic class, flow label, hop limit, addresses, ports,
    seq, ack, the reserved bits and flags next to the data offset, window,
    urgent pointer. field / ip4_field: the checksum fields' contents."""
    payload = bytes(payload)
    tags = [] if vlan is None else ([vlan] if isinstance(vlan, int) else list(vlan))
    if saturate:
        tags = [0xFFFF] * len(tags)
    ones = saturate
    if kind == "tcp":
        l4 = struct.pack(">HHIIBBHHH", 0xFFFF if ones else 40000, 0xFFFF if ones else 40001, M32 if ones else 1,
                         M32 if ones else 2, 0x5F if ones else 0x50, 0xFF if ones else 0x18,
                         0xFFFF if ones else 100, field, 0xFFFF if ones else 0)
        proto, foff = 6, 16
    else:
        assert kind == "udp" and 8 + len(payload) <= 0xFFFF
        l4 = struct.pack(">HHHH", 0xFFFF if ones else 40000, 0xFFFF if ones else 40001, 8 + len(payload), field)
        proto, foff = 17, 6
    seg = len(l4) + len(payload)
    if net == "ip4":
        assert len(options) % 4 == 0 and len(options) <= 40 and 20 + len(options) + seg <= 0xFFFF
        addr = (b"\xff" * 4, b"\xff" * 4) if ones else (b"\x0a\x00\x00\x01", b"\x0a\x00\x00\x02")
        ip = struct.pack(">BBHHHBBH4s4s", 0x40 | (5 + len(options) // 4), 0xFF if ones else 0,
                         20 + len(options) + seg, 0xFFFF if ones else 7, 0xC000 if ones else 0x4000,
                         0xFF if ones else 64, proto, ip4_field, *addr) + bytes(options)
        ethertype = 0x0800
    else:
        assert net == "ip6" and not options and seg <= 0xFFFF
        addr = (b"\xff" * 16, b"\xff" * 16) if ones else (bytes.fromhex("20010db8000000000000000000000001"),
                                                          bytes.fromhex("20010db8000000000000000000000002"))
        ip = struct.pack(">IHBB16s16s", 0x6FFFFFFF if ones else 0x60000000, seg, proto, 0xFF if ones else 64, *addr)
        ethertype = 0x86DD
    lk = _link(link, ethertype, tags, saturate)
    l3 = len(lk)
    o4 = l3 + len(ip)
    return Frame(lk + ip + l4 + payload, link=link, tags=len(tags), net=net, kind=kind, l3=l3, l4=o4,
                 seg_end=o4 + seg, field=o4 + foff, ip4_field=l3 + 10 if net == "ip4" else None,
                 payload=o4 + len(l4))


def udp_jumbogram(payload, link=None, saturate=False, sport=12345, dport=9999, checksum=0):
    """pktutil.ipv6_udp_jumbogram(hbh16=True) with any payload: IPv6 Length 0,
    a 16-byte HopByHop header (PadN, the Jumbo TLV, PadN) whose bytes 4-5 are 0,
    UDP with Length 0. IPv6.DecodeFromBytes keeps the HopByHop header in the
    jumbogram's Payload (ip6.go:249-256) and names its NextHeader as the next
    type, so the UDP decoder reads the HopByHop bytes as its header: Length 0
    (jumbo: the whole rest), Checksum 0xC204 (the TLV's type and length), and
    the summed segment is 16 + 8 + len(payload) bytes. The only way the decoded
    path sums a segment of 65 536 bytes or more."""
    payload = bytes(payload)
    hbh = bytes([17, 1, 1, 2, 0, 0, 0xC2, 4]) + struct.pack(">I", 16 + 8 + len(payload)) + bytes([1, 2, 0, 0])
    if saturate:
        sport = dport = 0xFFFF
    udp = struct.pack(">HHHH", sport, dport, 0, checksum)
    addr = (b"\xff" * 16, b"\xff" * 16) if saturate else (bytes.fromhex("20010db8000000000000000000000001"),
                                                          bytes.fromhex("20010db8000000000000000000000002"))
    ip = struct.pack(">IHBB16s16s", 0x6FFFFFFF if saturate else 0x60000000, 0, 0, 0xFF if saturate else 64, *addr)
    lk = _link(link, 0x86DD, [], saturate)
    l3 = len(lk)
    o4 = l3 + 40
    return Frame(lk + ip + hbh + udp + payload, link=link, tags=0, net="ip6", kind="udp", l3=l3, l4=o4,
                 seg_end=o4 + 24 + len(payload), field=o4 + 6, ip4_field=None, payload=o4 + 8)


# ---- the reference's arithmetic, restated -----------------------------------------

def go_compute_checksum(data, csum):
    """gopacket.ComputeChecksum (checksum.go:35-50): two additions per word
    into a uint32, an odd last byte counts << 8."""
    length = len(data) - 1
    for i in range(0, length, 2):
        csum = (csum + (data[i] << 8)) & M32
        csum = (csum + data[i + 1]) & M32
    if len(data) % 2 == 1:
        csum = (csum + (data[length] << 8)) & M32
    return csum


def go_fold_checksum(csum):
    """gopacket.FoldChecksum (checksum.go:53-58); the same loop folds a big integer."""
    while csum > 0xFFFF:
        csum = (csum >> 16) + (csum & 0xFFFF)
    return ~csum & 0xFFFF


Csum = collections.namedtuple("Csum", "csum valid field sum32 sum_big csum_big")
Csum.__doc__ = """csum: the reference's Correct (FoldChecksum(verification - existing) in uint32); valid: its
Valid; field: Actual; sum32: verification as the uint32 the reference holds; sum_big: the same sum in
unbounded integers; csum_big: the fold of sum_big - existing, the RFC 1071 value. Every wrap of the
uint32 loses 2^32 = 1 (mod 65535), so csum differs from csum_big once sum_big passes 2^32."""


def _word_sum_big(data):
    """Sum of the big-endian 16-bit words of data, unbounded (an odd last byte << 8)."""
    a = np.frombuffer(bytes(data), np.uint8)
    return 256 * int(a[0::2].sum(dtype=np.uint64)) + int(a[1::2].sum(dtype=np.uint64))


def py_checksums(packet_bytes, layout, kind):
    """What the reference's VerifyChecksum gives for one packet, from its bytes
    and its layer slices (layout["start"][slot], layout["end"][slot]).
    kind "ip4": IPv4.VerifyChecksum (ip4.go:323-332) over Contents (IHL * 4 bytes);
    kind "tcp" / "udp": tcpipchecksum.computeChecksum (tcpip.go:54-69) with the
    pseudo-header of the packet's network layer, over the TCP slice, or over UDP's
    Contents + Payload (udp.go:41-51: Length bytes, cut to the slice; Length 0: the
    whole slice), and UDP.VerifyChecksum's field-0 rule (udp.go:144-158).
    Returns a Csum."""
    b = bytes(packet_bytes)
    start, end = layout["start"], layout["end"]
    if kind == "ip4":
        s = int(start[IP4])
        data = b[s:s + 4 * (b[s] & 0x0F)]
        existing = data[10] << 8 | data[11]
        csum, big = 0, 0
    else:
        v4, v6 = int(start[IP4]) != ABSENT, int(start[IP6]) != ABSENT
        assert v4 != v6, "one network layer"
        csum = 0
        if v4:  # tcpip.go:26-35
            ip = b[int(start[IP4]):]
            src, dst = ip[12:16], ip[16:20]
            csum = (csum + ((src[0] + src[2]) << 8)) & M32
            csum = (csum + src[1] + src[3]) & M32
            csum = (csum + ((dst[0] + dst[2]) << 8)) & M32
            csum = (csum + dst[1] + dst[3]) & M32
            big = _word_sum_big(src + dst)
        else:  # tcpip.go:37-48
            ip = b[int(start[IP6]):]
            src, dst = ip[8:24], ip[24:40]
            for i in range(0, 16, 2):
                csum = (csum + (src[i] << 8)) & M32
                csum = (csum + src[i + 1]) & M32
                csum = (csum + (dst[i] << 8)) & M32
                csum = (csum + dst[i + 1]) & M32
            big = _word_sum_big(src + dst)
        if kind == "tcp":
            data = b[int(start[TCP]):int(end[TCP])]
            existing = data[16] << 8 | data[17]
            proto = 6
        else:
            assert kind == "udp"
            data = b[int(start[UDP]):int(end[UDP])]
            length = data[4] << 8 | data[5]
            assert length == 0 or length >= 8
            if length:
                data = data[:min(length, len(data))]
            existing = data[6] << 8 | data[7]
            proto = 17
        n = len(data)
        csum = (csum + proto) & M32
        csum = (csum + (n & 0xFFFF)) & M32
        csum = (csum + (n >> 16)) & M32
        big += proto + (n & 0xFFFF) + (n >> 16)
    sum32 = go_compute_checksum(data, csum)
    big += _word_sum_big(data)
    correct = go_fold_checksum((sum32 - existing) & M32)
    valid = correct == existing or (kind == "udp" and existing == 0)
    return Csum(correct, valid, existing, sum32, big, go_fold_checksum(big - existing))


def steer(frame_, field_offset, target=None, kind=None):
    """The frame with one 16-bit word rewritten so that the reference computes
    what the test wants (checked with py_checksums before it is returned).
    target None: field_offset is a checksum field (frame.field or
    frame.ip4_field), which is set to the computed value: a valid packet. The
    computed value does not depend on the field (it is subtracted again).
    target 0..0xFFFE: field_offset is any other word the sum covers at word
    alignment (two payload bytes, a header field, an address word of the
    pseudo-header); it is set so that the computed checksum is `target`. 0xFFFF
    cannot be computed: it needs a zero sum.
    kind: which checksum is steered; by default the IPv4 header's for a word of
    its first 12 bytes, else the transport layer's."""
    f = frame_
    if kind is None:
        kind = "ip4" if f.ip4_field is not None and f.l3 <= field_offset < f.l3 + 12 else f.kind
    own = f.ip4_field if kind == "ip4" else f.field
    b = bytearray(f)
    lay = f.layout()
    if target is None:
        assert field_offset == own, "steer: not the checksum field"
        c = py_checksums(b, lay, kind).csum
        struct.pack_into(">H", b, field_offset, c)
        got = py_checksums(b, lay, kind)
        assert got.valid and got.csum == got.field == c, "steer: the field moved the computed value"
        return f.replace(b)
    assert 0 <= target < 0xFFFF and field_offset != own
    base = f.l3 if (kind == "ip4" or field_offset < f.l4) else f.l4
    assert (field_offset - base) % 2 == 0, "steer: the word is not aligned to the sum's words"
    struct.pack_into(">H", b, field_offset, 0)
    c0 = py_checksums(b, lay, kind)
    assert c0.sum32 == c0.sum_big, "steer: the sum wraps"
    x0 = c0.sum32 - c0.field
    t = ~target & 0xFFFF  # the folded sum wanted, 1..0xFFFF; the fold of x > 0 is (x - 1) % 65535 + 1
    struct.pack_into(">H", b, field_offset, (t - x0) % 65535)
    got = py_checksums(b, lay, kind)
    assert got.csum == target and got.field == c0.field, (got, target)
    return f.replace(b)


def steer_two_folds(frame_, field_offset, kind=None):
    """The frame with the word at field_offset (as steer's: aligned, not the
    checksum field) rewritten so that FoldChecksum needs its second iteration:
    the low half of verification - existing becomes 0xFFFF under a high half
    h >= 1 (0x0001FFFF -> 0x00010000 -> 0x0001), so the computed value is ~h.
    None when the sum cannot reach 2^16."""
    f = frame_
    if kind is None:
        kind = "ip4" if f.ip4_field is not None and f.l3 <= field_offset < f.l3 + 12 else f.kind
    assert field_offset != (f.ip4_field if kind == "ip4" else f.field)
    base = f.l3 if (kind == "ip4" or field_offset < f.l4) else f.l4
    assert (field_offset - base) % 2 == 0, "steer: the word is not aligned to the sum's words"
    b = bytearray(f)
    lay = f.layout()
    struct.pack_into(">H", b, field_offset, 0)
    c0 = py_checksums(b, lay, kind)
    assert c0.sum32 == c0.sum_big, "steer: the sum wraps"
    x0 = c0.sum32 - c0.field
    x = x0 + ((0xFFFF - x0) & 0xFFFF)
    if x >> 16 == 0:
        return None
    struct.pack_into(">H", b, field_offset, x - x0)
    got = py_checksums(b, lay, kind)
    assert got.sum32 - got.field == x and x & 0xFFFF == 0xFFFF and got.csum == ~(x >> 16) & 0xFFFF, got
    return f.replace(b)


# ---- batches with explicit placement ------------------------------------------------

class Batch:
    """Packets placed one after another at chosen addresses (never overlapping,
    offsets ascending); finish() gives the (data, offsets, caplens) of
    pktutil.pack, 64 zero bytes after the last packet included."""

    def __init__(self):
        self.packets, self.offsets, self.cur = [], [], 0

    def __len__(self):
        return len(self.packets)

    def place(self, pkt, at=None):
        at = self.cur if at is None else at
        assert at >= self.cur
        self.packets.append(pkt)
        self.offsets.append(at)
        self.cur = at + len(pkt)
        return len(self.packets) - 1

    def phase(self, p, mod=16):
        """The next packet goes to the next address congruent to p modulo mod."""
        self.cur += (p - self.cur) % mod

    def gap(self, n):
        self.cur += n

    def fill_wave(self, pkt):
        """Copies of pkt up to the next multiple of 64 packets (b"": lanes without any bytes)."""
        while len(self.packets) % WAVE:
            self.place(pkt)

    def segments(self):
        """(start, end) of every packet's summed segment inside the packet; None for bytes that are no Frame."""
        return [p.segment() if isinstance(p, Frame) else None for p in self.packets]

    def extents(self):
        return [(0, len(p)) for p in self.packets]

    def finish(self, slack=0):
        data = np.zeros(self.cur + 64 + slack, np.uint8)
        for o, p in zip(self.offsets, self.packets):
            if len(p):
                data[o:o + len(p)] = np.frombuffer(p, np.uint8)
        return data, np.array(self.offsets, np.uint64), np.array([len(p) for p in self.packets], np.uint32)


_fillers = {}


def filler(link):
    """A valid 60-byte packet: Ethernet/IPv4/TCP with 6 payload bytes, or (link None) IPv6/UDP with 12."""
    if link not in _fillers:
        if link == "eth":
            f = frame("ip4", "tcp", b"filler")
            f = steer(f, f.ip4_field)
        else:
            f = frame("ip6", "udp", b"filler678901", link=None)
        _fillers[link] = steer(f, f.field)
        assert len(_fillers[link]) == 60
    return _fillers[link]


BANDS = {"small": (0, 256), "mid": (256, 1024), "big": (1024, 1 << 62)}  # mean packet: buffer bytes / packets


def to_band(batch, band, link):
    """The batch (a whole number of waves) with its mean packet (data bytes /
    packets, what selects the decode kernel) inside `band`: whole waves of
    60-byte fillers after it bring the mean down, unused zero bytes after the
    last packet bring it up. The waves of the batch itself stay as they are."""
    assert len(batch) % WAVE == 0
    lo, hi = BANDS[band]
    b = Batch()
    b.packets, b.offsets, b.cur = list(batch.packets), list(batch.offsets), batch.cur
    fill = filler(link)
    while (b.cur + 64) // len(b) >= hi:
        need = (b.cur + 64 - hi * len(b)) // (hi - 60) + 1  # fillers until the mean is under hi
        for _ in range((need + WAVE - 1) // WAVE * WAVE):
            b.place(fill)
    slack = max(0, lo * len(b) - (b.cur + 64))
    data, off, cap = b.finish(slack)
    assert lo <= len(data) // len(off) < hi, (band, len(data), len(off))
    return data, off, cap


# ---- dense_region, restated ---------------------------------------------------------

def wave_plan(offsets, segments):
    """gpk_kernels.hip dense_region over each group of 64 consecutive packets:
    the job lanes' byte ranges (segments[i] = (start, end) inside packet i, None
    = no job) form a dense region when none is longer than 65 536 bytes, all lie
    within +-2 GiB of the first job's chunk, and hi - lo16 <= 4 * tot + 8192.
    Returns one dict per wave: dense, far, R0 (the region's 16-byte-aligned
    base), R (its length), tot, jobs. The decode kernels apply it to the
    packets' extents (stream before the parse, early stream start) and to the
    L4 segments (after the parse)."""
    out = []
    for w in range(0, len(offsets), WAVE):
        jobs = [(int(o) + s[0], int(o) + s[1]) for o, s in zip(offsets[w:w + WAVE], segments[w:w + WAVE])
                if s is not None]
        if not jobs:
            out.append(dict(dense=False, far=False, R0=0, R=0, tot=0, jobs=0))
            continue
        base = jobs[0][0] & ~15
        far = any(not (-(1 << 31) <= s - base < (1 << 31)) or not (-(1 << 31) <= e - base < (1 << 31)) or
                  e - s > 65536 for s, e in jobs)
        lo, hi = min(s for s, _ in jobs), max(e for _, e in jobs)
        tot = sum(e - s for s, e in jobs) & M32
        lo16 = lo & ~15
        dense = not far and hi - lo16 <= ((4 * tot + 8192) & M32)
        out.append(dict(dense=dense, far=far, R0=lo16, R=hi - lo16, tot=tot, jobs=len(jobs)))
    return out


def region_lsum(data, R0, upto):
    """The dense stream's prefix before address `upto`, unbounded: the L-form
    sum (little-endian 16-bit words at even addresses, i.e. even-address bytes
    + 256 * odd-address bytes) of data[R0:upto]."""
    a = np.asarray(data[R0:upto], np.uint8)
    odd = (np.arange(R0, upto) & 1).astype(bool)
    return int(a[~odd].sum(dtype=np.uint64)) + 256 * int(a[odd].sum(dtype=np.uint64))


# ---- the case families ----------------------------------------------------------------

# A. a wave of saturated frames
A_PATTERNS = ("ff", "zero_ffff", "alt")
A_PHASE_GROUPS = [(p, p + 1) for p in range(0, 16, 2)]


@functools.lru_cache(maxsize=None)
def saturated_frames(pattern):
    """64 TCP/IPv4 frames, saturate=True, 2 400 payload bytes each: 0xFF; 0x00
    under a checksum field of 0xFFFF; or FF 00 ... and 00 FF ... in turn."""
    if pattern == "ff":
        return [frame("ip4", "tcp", b"\xff" * 2400, saturate=True)] * WAVE
    if pattern == "zero_ffff":
        return [frame("ip4", "tcp", bytes(2400), saturate=True, field=0xFFFF)] * WAVE
    assert pattern == "alt"
    two = [frame("ip4", "tcp", pay * 1200, saturate=True) for pay in (b"\xff\x00", b"\x00\xff")]
    return [two[i & 1] for i in range(WAVE)]


@functools.lru_cache(maxsize=None)
def family_a(pattern, phases):
    """Per phase p: the 64 frames packed from an address = p (mod 16) at batch
    indices that are one whole wave, then again (after 32 fillers) across two
    waves, each half saturated frames and half fillers. Returns the batch and,
    per phase, the index of the whole wave's first frame."""
    b, fill, frames, whole = Batch(), filler("eth"), saturated_frames(pattern), []
    for _ in range(WAVE):
        b.place(fill)
    for p in phases:
        b.phase(p)
        whole.append(len(b))
        for f in frames:
            b.place(f)
        for _ in range(32):
            b.place(fill)
        b.phase(p)
        assert len(b) % WAVE == 32
        for f in frames:
            b.place(f)
        b.fill_wave(fill)
    return b, whole


# B. residues and validity
B_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025)
B_PATTERNS = ("zero", "ff", "alt", "last01")


def b_payload(pattern, n):
    if pattern == "zero":
        return bytes(n)
    if pattern == "ff":
        return b"\xff" * n
    if pattern == "alt":
        return (b"\xff\x00" * (n // 2 + 1))[:n]
    assert pattern == "last01"
    return bytes(max(0, n - 1)) + b"\x01" * min(1, n)


def _l4_free_word(f):
    """A word of the L4 sum that no decoder reads: the first two payload bytes,
    else TCP's window, else (UDP without two payload bytes) the source address's last word."""
    if f.seg_end - f.payload >= 2:
        return f.payload
    if f.kind == "tcp":
        return f.l4 + 14
    return f.l3 + (14 if f.net == "ip4" else 22)


@functools.lru_cache(maxsize=None)
def residue_frames(link):
    """(label, frame) for every payload pattern, length, network and transport
    layer, each as: checksum field 0 (UDP: valid by rule), the computed value
    steered to 0x0000 under a field of 0 (valid) and of 0x1234 (not), the field
    steered to the computed value (valid), the sum steered so that the fold needs
    its second iteration (where the sum reaches 2^16), and for the zero payload
    a field of 0xFFFF. link None: the IPv6 ones, bare."""
    out = []
    for net in (("ip4", "ip6") if link == "eth" else ("ip6",)):
        for kind in ("tcp", "udp"):
            for pat in B_PATTERNS:
                for n in B_LENGTHS:
                    what = "%s/%s/%s/%d" % (net, kind, pat, n)
                    base = frame(net, kind, b_payload(pat, n), link=link)
                    out.append((what + "/field0", base))
                    zero = steer(base, _l4_free_word(base), 0x0000)
                    out.append((what + "/computed0", zero))
                    out.append((what + "/valid", steer(base, base.field)))
                    other = frame(net, kind, b_payload(pat, n), link=link, field=0x1234)
                    out.append((what + "/computed0-field1234", steer(other, _l4_free_word(other), 0x0000)))
                    two = steer_two_folds(base, _l4_free_word(base))
                    if two is not None:
                        out.append((what + "/twofold", two))
                    if pat == "zero":
                        out.append((what + "/fieldffff", frame(net, kind, b_payload(pat, n), link=link, field=0xFFFF)))
    return out


OPTIONS_FF = {"kind_ff_len_40": b"\xff\x28" + b"\xff" * 38,  # one option of kind 0xFF, length 40
              "all_ff": b"\xff" * 40}                         # kind 0xFF, length 0xFF: exceeds the header


def ip4_header_frames():
    """(label, frame): IPv4 headers at their ends. Saturated 20-byte headers;
    IHL 15 with 40 option bytes of 0xFF (both ways to write them: the oracle
    decides which carry GPK_ST_IP4_CSUM); each with the header checksum steered
    to valid, the computed value steered (through Id) to 0x0000 under a field of
    0 and of 0x1234, the two-iteration fold, and a field of 0xFFFF."""
    out = []
    for sat in (False, True):
        for oname, opts in [("none", b"")] + sorted(OPTIONS_FF.items()):
            what = "ip4hdr/%s/%s" % ("saturated" if sat else "plain", oname)
            base = frame("ip4", "tcp", b"\xff" * 32, options=opts, saturate=sat)
            out.append((what + "/field0", base))
            out.append((what + "/valid", steer(base, base.ip4_field)))
            zero = steer(base, base.l3 + 4, 0x0000)
            out.append((what + "/computed0", zero))
            other = frame("ip4", "tcp", b"\xff" * 32, options=opts, saturate=sat, ip4_field=0x1234)
            out.append((what + "/computed0-field1234", steer(other, other.l3 + 4, 0x0000)))
            two = steer_two_folds(base, base.l3 + 4)
            if two is not None:
                out.append((what + "/twofold", two))
            out.append((what + "/fieldffff", frame("ip4", "tcp", b"\xff" * 32, options=opts, saturate=sat,
                                                   ip4_field=0xFFFF)))
    return out


def window_edge_frames():
    """(label, frame): a saturated IPv4 header behind 11..20 stacked 802.1Q tags,
    so that it starts at packet byte 58..94 and, depending on the packet's
    address, ends inside or past the lane's header window (96 bytes from the
    packet's 16-byte chunk; 80 in the dword-aligned kernel): sum_words_lds<20>
    on one side, the general sum_words on the other. With and without the 0xFF options."""
    out = []
    for ntags in range(11, 21):
        for oname, opts in (("none", b""), ("kind_ff_len_40", OPTIONS_FF["kind_ff_len_40"])):
            f = frame("ip4", "tcp", b"\xff" * 20, vlan=[1] * ntags, options=opts, saturate=True)
            out.append(("winedge/%dtags/%s" % (ntags, oname), steer(f, f.ip4_field)))
    return out


@functools.lru_cache(maxsize=None)
def family_b(link):
    """Every residue frame at an even and at an odd batch address, the IPv4
    header frames likewise, the window-edge frames at all 16 byte phases.
    Returns the batch and the labels of its packets (None: a filler)."""
    b, labels, fill = Batch(), [], filler(link)
    cases = residue_frames(link) + (ip4_header_frames() if link == "eth" else [])
    for parity in (0, 1):
        for what, f in cases:
            b.phase(parity, 2)
            b.place(f)
            labels.append("%s@%s" % (what, "odd" if parity else "even"))
    if link == "eth":
        for what, f in window_edge_frames():
            for p in range(16):
                b.phase(p)
                b.place(f)
                labels.append("%s@%d" % (what, p))
    b.fill_wave(fill)
    labels += [None] * (len(b) - len(labels))
    return b, labels


# C. length limits
@functools.lru_cache(maxsize=None)
def limit_frame(kind, link):
    """tcp4: TCP/IPv4 with the longest segment IPv4's Length allows (65 515);
    tcp6: TCP/IPv6 with Length 65 535; j65536 / j65537: the UDP jumbogram form
    with a summed segment of 65 536 (still dense) / 65 537 bytes (sparse by the
    length rule); x65536 / x65537: TCP/IPv4 frames of 65 536 / 65 537 bytes in
    all (the same rule on the packets' extents, which the stream before the
    parse and the early stream start go by). All 0xFF, saturate=True."""
    if kind == "tcp4":
        f = frame("ip4", "tcp", b"\xff" * (65515 - 20), link=link, saturate=True)
        assert f.seg_end - f.l4 == 65515
    elif kind == "tcp6":
        f = frame("ip6", "tcp", b"\xff" * (65535 - 20), link=link, saturate=True)
        assert f.seg_end - f.l4 == 65535
    elif kind in ("j65536", "j65537"):
        f = udp_jumbogram(b"\xff" * (int(kind[1:]) - 24), link=link, saturate=True)
        assert f.seg_end - f.l4 == int(kind[1:])
    else:
        assert kind in ("x65536", "x65537") and link == "eth"
        f = frame("ip4", "tcp", b"\xff" * (int(kind[1:]) - 54), link=link, saturate=True)
        assert len(f) == int(kind[1:])
    return f


C_KINDS = {"eth": ("tcp4", "tcp6", "j65536", "j65537", "x65536", "x65537"), None: ("tcp6", "j65536", "j65537")}


@functools.lru_cache(maxsize=None)
def family_c(kind, link):
    """Four waves: the frame at an even and at an odd address, alone in its wave
    (the other 63 lanes hold no bytes), then each again followed by 63 packed
    60-byte neighbours. Returns the batch and the four waves' first indices."""
    b, f, fill, first = Batch(), limit_frame(kind, link), filler(link), []
    for neighbours in (b"", fill):
        for parity in (0, 1):
            b.phase(parity, 2)
            first.append(len(b))
            b.place(f)
            b.fill_wave(neighbours)
    return b, first


# D. the reference's uint32 wrap
D_PAYLOADS = (131100, 262080)


@functools.lru_cache(maxsize=None)
def family_d(link=None):
    """The jumbogram form with 131 100 and 262 080 payload bytes of 0xFF (a
    packet of 262 144 bytes), each at an even and an odd address, each followed
    by 63 fillers. Returns the batch and the four frames' indices."""
    b, fill, first = Batch(), filler(link), []
    for n in D_PAYLOADS:
        f = udp_jumbogram(b"\xff" * n, link=link)
        for parity in (0, 1):
            b.phase(parity, 2)
            first.append(len(b))
            b.place(f)
            b.fill_wave(fill)
    return b, first


# E. the dense / sparse predicate at its threshold
def boundary_wave(gap, frames, split=32):
    b = Batch()
    b.phase(5)  # lo16 is below the first byte: the rounding is part of the predicate
    for i, f in enumerate(frames):
        if i == split:
            b.gap(gap)
        b.place(f)
    return b


def boundary_gap(frames, ranges):
    """The largest gap (between the 32nd and the 33rd frame) at which the wave is
    still dense by wave_plan over `ranges` ("segments" or "extents")."""
    def dense(g):
        b = boundary_wave(g, frames)
        return wave_plan(b.offsets, getattr(b, ranges)())[0]["dense"]
    lo, hi = 0, 1 << 22
    assert dense(lo) and not dense(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if dense(mid):
            lo = mid
        else:
            hi = mid
    return lo


@functools.lru_cache(maxsize=None)
def family_e(ranges):
    """64 saturated TCP/IPv4 frames with 600-byte segments of 0xFF at explicit
    offsets, three times: with the largest gap g that keeps the wave dense, with
    g + 1 and with g + 16 (not dense). Apart from the offsets the waves hold the
    same packets. Returns the batch and g."""
    frames = [frame("ip4", "tcp", b"\xff" * 580, saturate=True)] * WAVE
    g = boundary_gap(frames, ranges)
    b = Batch()
    for gap in (g, g + 1, g + 16):
        w = boundary_wave(gap, frames)
        base = (b.cur + 15) & ~15
        for o, f in zip(w.offsets, w.packets):
            b.place(f, base + o)
        b.gap(64)
    return b, g
