"""Cases for the capture writers' batch path (include/gpk_capwrite.h), shared
by the host test (gpk_capwrite_batch_host) and the device test: the smallest
shapes at which the framing can still go wrong.

alignment_case(): every capture length of 0..70 and 1490..1530 (every residue
mod 4 and mod 16, empty packets, the 16-byte head-only and tail-only copies,
MTU-sized packets that take more than one pass of a 16-lane group) at each of
the 16 source alignments: 1792 packets. The caller runs it at 16 output base
offsets, so every length meets every source and destination alignment.
Scattered through it: both kinds of error packets, every special timestamp,
and option blobs of 0, 4 and 40 bytes."""
import numpy as np

from gopacket_amd import _lib

import capwrite_model as M

CAPLENS = list(range(0, 71)) + list(range(1490, 1531))
TIMES = [(0, 0), (-1000, 5), M.ZERO, (1, 999999999), ((1 << 32) + 5, 1), (1519128000, 195312500),
         (-62135596800, 1), (1 << 40, 7), (-(1 << 35), 999999999)]
NOW = (1700000000, 123456789)
INTERFACES = 2
OPT4 = bytes(4)                                                   # end-of-options alone
OPT40 = b"\x01\x00\x1d\x00" + b"a comment of 29 bytes, padded" + bytes(3) + bytes(4)
assert len(OPT40) == 40


def make_batch(specs, seed=7):
    """specs: [(caplen, source alignment mod 16)]. Packets lie apart, each at
    its alignment, random bytes between them."""
    rng = np.random.default_rng(seed)
    offs, pos = [], 32
    for caplen, a in specs:
        pos = (pos + 15) // 16 * 16 + a
        offs.append(pos)
        pos += caplen + int(rng.integers(0, 5))
    data = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    offsets = np.array(offs, np.uint64)
    caplens = np.array([c for c, _ in specs], np.uint32)
    packets = [bytes(data[o:o + c]) for o, c in zip(offs, caplens.tolist())]
    return data, offsets, caplens, packets


def capture_infos(caplens, errors=True):
    """One gpk_capture_info per packet: timestamps cycle through TIMES, the
    wire length is the capture length plus 0..2, interfaces alternate; with
    errors every 37th packet has caplen > length and every 41st an interface
    the writer does not have (2 or -1)."""
    n = len(caplens)
    ci = np.zeros(n, _lib.CAPINFO_DTYPE)
    for k in range(n):
        sec, nsec = TIMES[k % len(TIMES)]
        length, iface = int(caplens[k]) + k % 3, k % INTERFACES
        if errors and k % 37 == 5 and caplens[k] > 0:
            length = int(caplens[k]) - 1
        if errors and k % 41 == 7:
            iface = 2 if k % 2 else -1
        ci[k] = (sec, nsec, length, iface, -1)
    return ci


def ci_tuples(ci):
    return [(int(r["ts_sec"]), int(r["ts_nsec"]), int(r["length"]), int(r["iface"])) for r in ci]


def option_blobs(m):
    """Per output packet: none for most, 4 and 40 bytes mixed in."""
    return [OPT4 if j % 5 == 1 else OPT40 if j % 7 == 3 else None for j in range(m)]


def pack_options(blobs):
    """(opt_data uint8 with 16 spare bytes, opt_off uint64[m+1]) of option_blobs()."""
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b or b"") for b in blobs], dtype=np.uint64)
    return np.frombuffer(b"".join(b or b"" for b in blobs) + bytes(16), np.uint8).copy(), off


def alignment_case():
    specs = [(c, a) for c in CAPLENS for a in range(16)]
    data, offsets, caplens, packets = make_batch(specs)
    return dict(data=data, offsets=offsets, caplens=caplens, packets=packets, ci=capture_infos(caplens))


def orders(n, seed=3):
    """order = NULL, a permutation, a selection with repeats."""
    rng = np.random.default_rng(seed)
    return dict(none=None, permutation=rng.permutation(n).astype(np.uint32),
                repeats=np.sort(rng.integers(0, n, n // 3)).astype(np.uint32)[::-1].copy())


def big_case():
    """One packet of 65 535 bytes and one of 262 144 among small neighbours."""
    specs = [(60, 3), (65535, 5), (0, 0), (262144, 11), (1500, 9), (33, 15)]
    data, offsets, caplens, packets = make_batch(specs, seed=11)
    return dict(data=data, offsets=offsets, caplens=caplens, packets=packets, ci=capture_infos(caplens, errors=False))


def expected(fmt, case, order=None, blobs=None, out_cap=None):
    """The model's (bytes of out[:needed], block_off, status, counts)."""
    blocks, off, status, counts = M.frame_batch(fmt, INTERFACES, case["packets"], ci_tuples(case["ci"]),
                                                None if order is None else order.tolist(), blobs, NOW, out_cap)
    return b"".join(blocks), off, status, counts
