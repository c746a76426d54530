"""Batches for the big-packet L4 kernel's stream-windows body
(gpk_kernels.hip decode_sw_body): the header windows are taken out of the
checksum stream, so every case here is about where a packet's window lies in
the stream's passes, or about a wave that must not take that path.

wave_path restates the body's arithmetic in Python (as csumcases.wave_plan
restates dense_region, which it builds on) and is used only to assert that a
case is what it claims to be; test_stream_windows_cpu.py does that and pins the
oracle on the same batches, test_stream_windows_gpu.py compares the device.
"""
import functools
import struct

import numpy as np

import csumcases as C

WAVE = 64
CELLS = 6        # 16-byte cells of a header window
PASS = 64        # granules of one stream pass (one per lane)


class Case:
    """name, the batch (data, off, cap), the parsers it runs under, and what
    the CPU test asserts about it (claims: a dict the builders fill)."""

    def __init__(self, name, data, off, cap, packets, parsers=("eth_ip4_tcp_payload", "statsassembly"), **claims):
        self.name, self.data, self.off, self.cap, self.packets = name, data, off, cap, packets
        self.parsers, self.claims = parsers, claims

    @property
    def batch(self):
        return self.data, self.off, self.cap


# ---- frames -------------------------------------------------------------------------

def _words(b):
    a = np.frombuffer(bytes(b) + (b"\x00" if len(b) & 1 else b""), np.uint8).astype(np.uint64)
    return int(256 * a[0::2].sum() + a[1::2].sum())


def _fold(x):
    while x > 0xFFFF:
        x = (x >> 16) + (x & 0xFFFF)
    return ~x & 0xFFFF


def validate(f):
    """The frame with both checksum fields set to what the reference computes
    (sums of at most 9 000 bytes never wrap; the CPU test checks the result
    against csumcases.py_checksums)."""
    b = bytearray(f)
    ihl = 4 * (b[f.l3] & 15)
    struct.pack_into(">H", b, f.ip4_field, 0)
    struct.pack_into(">H", b, f.ip4_field, _fold(_words(b[f.l3:f.l3 + ihl])))
    struct.pack_into(">H", b, f.field, 0)
    seg = b[f.l4:f.seg_end]
    struct.pack_into(">H", b, f.field, _fold(_words(b[f.l3 + 12:f.l3 + 20]) + 6 + len(seg) + _words(seg)))
    return f.replace(b)


def tcp_options(f, n):
    """The TCP/IPv4 frame with n bytes (a multiple of 4, at most 40) of NOP options."""
    assert f.kind == "tcp" and f.net == "ip4" and n % 4 == 0 and n <= 40
    b = bytearray(f)
    b[f.l4 + 20:f.l4 + 20] = b"\x01" * n
    b[f.l4 + 12] = (5 + n // 4) << 4 | (b[f.l4 + 12] & 15)
    struct.pack_into(">H", b, f.l3 + 2, struct.unpack_from(">H", b, f.l3 + 2)[0] + n)
    w = dict(f.__dict__)
    w.update(seg_end=f.seg_end + n, payload=f.payload + n)
    return C.Frame(bytes(b), **w)


@functools.lru_cache(maxsize=None)
def tcp_frame(length, seed=0, valid=True):
    """Ethernet/IPv4/TCP of `length` bytes in all (54 of headers), seeded random payload."""
    pay = np.random.default_rng(1000 + seed).integers(0, 256, length - 54, dtype=np.uint8).tobytes()
    f = C.frame("ip4", "tcp", pay)
    assert len(f) == length
    return validate(f) if valid else f


@functools.lru_cache(maxsize=None)
def long_header_frame(length=1500):
    """QinQ + IPv4 with 40 bytes of options + TCP with 40 bytes of options: 142
    bytes of headers, past any 96-byte window."""
    pay = np.random.default_rng(77).integers(0, 256, length - 142, dtype=np.uint8).tobytes()
    f = tcp_options(C.frame("ip4", "tcp", pay, vlan=[0x0123, 0x0456], options=b"\x01" * 40), 40)
    assert len(f) == length and f.l3 == 22 and f.l4 == 82 and f.payload == 142
    return validate(f)


# ---- placement ----------------------------------------------------------------------

class Placed:
    """Packets at chosen addresses (ascending in memory) and the index order
    they are handed over in, which the fallback cases permute."""

    def __init__(self):
        self.b = C.Batch()
        self.caps = []

    def place(self, pkt, cap=None):
        """cap: the caplen handed over (a cut packet still occupies its bytes)."""
        i = self.b.place(pkt)
        self.caps.append(len(pkt) if cap is None else cap)
        return i

    def finish(self, order=None):
        data, off, _ = self.b.finish()
        cap = np.array(self.caps, np.uint32)
        pk = [p[:c] for p, c in zip(self.b.packets, self.caps)]
        if order is not None:
            off, cap, pk = off[order], cap[order], [pk[i] for i in order]
        return data, off, cap, pk


# ---- the body's arithmetic, restated ----------------------------------------------------

def window(off, cl):
    """win_geo<6, 16>: the window's first granule address and its cells."""
    m = int(off) & 15
    win = min(int(cl), 16 * CELLS - m)
    return int(off) - m, (m + win + 15) >> 4


def wave_path(off, cap):
    """Per wave of 64 packets: stream (the packets' extents are a dense region
    and the offsets do not decrease in lane order), dense, sorted, R0, and per
    packet (h, cells, residue of h in its pass, whether the window crosses into
    the next pass); h is relative to R0, as in the kernel."""
    plan = C.wave_plan(off, [(0, int(c)) for c in cap])
    out = []
    for w, pl in enumerate(plan):
        o, c = off[w * WAVE:(w + 1) * WAVE], cap[w * WAVE:(w + 1) * WAVE]
        srt = all(int(o[i]) <= int(o[i + 1]) for i in range(len(o) - 1))
        pk = []
        for oo, cc in zip(o, c):
            wb, nch = window(oo, cc)
            h = (wb - pl["R0"]) >> 4
            pk.append(dict(h=h, cells=nch, residue=h % PASS, crosses=nch > 0 and h % PASS + nch > PASS,
                           ends_at_edge=nch > 0 and h % PASS + nch == PASS))
        out.append(dict(stream=pl["dense"] and srt, dense=pl["dense"], sorted=srt, R0=pl["R0"], R=pl["R"], packets=pk))
    return out


# ---- 1. byte phases and start granules ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case_phases():
    """16 waves of 1500-byte packets, wave p's first packet at an address = p (mod 16)."""
    pl, f = Placed(), tcp_frame(1500)
    for p in range(16):
        pl.b.phase(p)
        for _ in range(WAVE):
            pl.place(f)
    data, off, cap, pk = pl.finish()
    return Case("phases", data, off, cap, pk, first_phases=[int(off[WAVE * p]) & 15 for p in range(16)])


@functools.lru_cache(maxsize=None)
def case_residues():
    """Two waves (the first 16-byte aligned, the second from phase 5) of
    1520-byte packets: each starts 95 granules after the one before, and 95 is
    odd, so the windows' start granules step through all 64 residues of a pass:
    windows that end exactly at a pass boundary (residue 58) and windows that
    cross it (59-63) among them."""
    pl = Placed()
    for p in (0, 5):
        pl.b.phase(p)
        for q in range(WAVE):
            pl.place(tcp_frame(1520, seed=q % 4))
    data, off, cap, pk = pl.finish()
    return Case("residues", data, off, cap, pk)


# ---- 2. several owners per pass -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case_owners():
    """Four waves of runs of short packets between 9000-byte ones (which keep
    the mean above 1 KiB): 60-90-byte frames, packets shorter than a granule,
    windows of fewer than six cells, windows that share granules, one packet
    with caplen 0."""
    pl = Placed()
    big = tcp_frame(9000, seed=9)
    zero = None
    for w in range(4):
        for q in range(WAVE):
            if q % 8 == 7:
                pl.place(big)
            elif w == 0:
                pl.place(tcp_frame(60 + (q * 5) % 31, seed=q % 3))        # 60..90 bytes
            elif w == 1:
                pl.place(tcp_frame(60, seed=1), cap=1 + (q * 3) % 15)      # shorter than one granule
            elif w == 2:
                if q == 20:
                    zero = pl.place(tcp_frame(60, seed=2), cap=0)
                else:
                    pl.place(tcp_frame(90, seed=2), cap=17 + (q * 7) % 64)  # 2..6 cells
            else:
                pl.place(tcp_frame(54 + q % 11, seed=q % 5, valid=q % 4 != 0))
    data, off, cap, pk = pl.finish()
    return Case("owners", data, off, cap, pk, zero=zero)


# ---- 3. batch edges -------------------------------------------------------------------------

EDGE_N = (1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def case_edge(n, short_last):
    """n 1500-byte packets from phase 3; short_last: the last one is cut to 20
    bytes and is the batch's last bytes, so its window's last cell is the
    region's last granule."""
    pl, f = Placed(), tcp_frame(1500, seed=3)
    pl.b.phase(3)
    for q in range(n):
        if short_last and q == n - 1:
            pl.place(f[:20])
        else:
            pl.place(f)
    data, off, cap, pk = pl.finish()
    if short_last and n == 1:  # one 20-byte packet: unused bytes after it keep the mean
        data = np.concatenate([data, np.zeros(1024, np.uint8)])
    return Case("edge n=%d%s" % (n, " short last" if short_last else ""), data, off, cap, pk)


# ---- 4. waves that must take the other path ----------------------------------------------------

FALLBACK_WAVES = ("sorted", "reversed", "shuffled", "equal", "one_pair", "gap_inside", "gap_past")


@functools.lru_cache(maxsize=None)
def case_fallback():
    """Seven waves of 64 1500-byte packets, packed in memory, handed over in
    order; reversed; shuffled; with runs of equal offsets (lanes naming the same
    packet: non-decreasing, so still streamed); with one adjacent pair swapped;
    and, in order again, with the largest gap in the middle that keeps the wave
    dense, and one byte more."""
    pl = Placed()
    order = []
    rng = np.random.default_rng(5)
    tot = 64 * 1500
    for w, kind in enumerate(FALLBACK_WAVES):
        pl.b.phase(7)
        first = len(pl.b)
        for q in range(WAVE):
            if kind.startswith("gap") and q == 32:
                # dense_region: hi - lo16 <= 4 * tot + 8192, lo16 = the wave's first address & ~15
                room = 4 * tot + 8192 - (tot + 7)
                pl.b.gap(room if kind == "gap_inside" else room + 1)
            pl.place(tcp_frame(1500, seed=q % 8))  # the same 64 frames in every wave
        idx = list(range(first, first + WAVE))
        if kind == "reversed":
            idx.reverse()
        elif kind == "shuffled":
            idx = list(rng.permutation(idx))
        elif kind == "equal":
            idx = [first + 4 * (q // 4) for q in range(WAVE)]  # four lanes per packet; the others are skipped
        elif kind == "one_pair":
            idx[40], idx[41] = idx[41], idx[40]
        order += idx
    data, off, cap, pk = pl.finish(order)
    return Case("fallback", data, off, cap, pk)


# ---- 5. headers beyond the window, truncation ----------------------------------------------------

CUTS = (0, 5, 13, 14, 16, 18, 21, 22, 30, 41, 42, 60, 81, 82, 90, 95, 96, 97, 101, 102, 120, 141, 142, 143, 200)


@functools.lru_cache(maxsize=None)
def case_long_headers():
    """Two waves of the 142-byte-header frame (QinQ, IPv4 and TCP options), the
    first whole, the second with caplens that cut inside every header (Ethernet
    14, tags 18 / 22, IPv4 42 / 82, TCP 102 / 142) on both sides of the 96-byte
    window; every cut packet still occupies its 1500 bytes."""
    pl, f = Placed(), long_header_frame()
    pl.b.phase(9)
    for q in range(WAVE):
        pl.place(f)
    for q in range(WAVE):
        pl.place(f, cap=CUTS[q % len(CUTS)] if q % 2 else None)
    data, off, cap, pk = pl.finish()
    return Case("long headers", data, off, cap, pk, parsers=("statsassembly",))


def all_cases():
    out = [case_phases(), case_residues(), case_owners()]
    out += [case_edge(n, s) for n in EDGE_N for s in (False, True)]
    return out + [case_fallback(), case_long_headers()]
