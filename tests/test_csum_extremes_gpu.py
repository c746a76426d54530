"""Device == oracle, bit for bit, on the checksum extremes of
tests/csumcases.py (test_csum_extremes_cpu.py pins the oracle on the same
batches and asserts that each is what it claims to be): a wave whose dense
prefix wraps 2^32, the residues at both ends of l_to_words' even-address
branch, the 64 KiB rule at 65 536 / 65 537 bytes, segments whose word sum wraps
the reference's uint32, and dense_region's predicate at its threshold.

Every family runs through each launch that has a phase B or consumes its
result: the plain 16-byte record (the kernel its batch's mean packet selects:
fillers and unused bytes after the family's own waves move the mean into each
band), with layouts, with fused fields, with fused connection keys, the narrow
record with its side array and with its compact list, and global tables."""
import numpy as np
import pytest

import csumcases as C
from configs import CONFIGS, assert_same, device_parser, oracle_parser
from test_gpu_parity import K_BIG, K_FIELDS, K_LAY, K_SB, K_W5
from test_narrow_compact_gpu import check_equal, compact_device
from test_narrow_gpu import narrow_device

pytestmark = pytest.mark.gpu

LINK_OF = {"eth_ip4_tcp_payload": "eth", "statsassembly": "eth", "raw_ip6": None}
# the bands in which a parser's plain launch changes kernel (a parser with an IPv6
# decoder takes the stream-before-parse kernel below 1 KiB whatever the mean)
BANDS_OF = {"eth_ip4_tcp_payload": ("small", "mid", "big"), "statsassembly": ("mid", "big"), "raw_ip6": ("mid", "big")}
ALL_FIVE = {K_W5, K_SB, K_BIG, K_LAY, K_FIELDS}


def plain_kernel(name, band):
    if band == "big":
        return K_BIG
    return K_W5 if name == "eth_ip4_tcp_payload" and band == "small" else K_SB


def keys_device(ctx, grouper, dp, data, off, cap):
    """gpk_decode_group_batch (fused connection keys): the decode's own outputs."""
    import torch
    from gopacket_amd import _lib, flows
    n = len(off)
    d = torch.from_numpy(data).cuda()
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    c = torch.from_numpy(cap.astype(np.int32)).cuda()
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    grouper.decode_group(ctx, dp, d, o, c, rec, err, fl, kind=flows.CONNECTION)
    torch.cuda.synchronize()
    return dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
                flows=fl.cpu().numpy().view(np.uint64), layouts=None)


def every_form(ctx, grouper, name, batch, band, what, seen):
    """One batch in one band under one parser through every launch form, each
    against the oracle. Returns (oracle results, the plain launch's results); the
    family's own packets come first in both."""
    from gopacket_amd import _lib
    data, off, cap = C.to_band(batch, band, LINK_OF[name])
    assert len(off) <= grouper.max_packets
    cfg = CONFIGS[name]
    dp, op = device_parser(cfg), oracle_parser(cfg)
    ref = op.decode(data, off, cap, nthreads=8, layouts=True)
    want = plain_kernel(name, band)
    # the plain record, compact tables then global tables
    assert ctx.kernel_name(dp, data, off, cap, layouts=False) == want % "true", what
    plain = ctx.decode_host(dp, data, off, cap, layouts=False)
    assert_same(plain, ref, what + "/plain")
    ctx.set_table_mode(_lib.TABLES_GLOBAL)
    try:
        assert ctx.kernel_name(dp, data, off, cap, layouts=False) == want % "false", what
        assert_same(ctx.decode_host(dp, data, off, cap, layouts=False), ref, what + "/plain, global tables")
    finally:
        ctx.set_table_mode(_lib.TABLES_AUTO)
    # with layouts; with fused fields
    assert ctx.kernel_name(dp, data, off, cap, layouts=True) == K_LAY % "true", what
    assert_same(ctx.decode_host(dp, data, off, cap, layouts=True), ref, what + "/layouts")
    assert ctx.kernel_name(dp, data, off, cap, layouts=_lib.NAME_FIELDS) == K_FIELDS % "true", what
    assert_same(ctx.decode_host(dp, data, off, cap, layouts=False, fields=True), ref, what + "/fields")
    # with fused connection keys
    assert_same(keys_device(ctx, grouper, dp, data, off, cap), ref, what + "/keys")
    # the narrow record: side array, then compact list; the widened set is the oracle's
    nref = op.decode_narrow(data, off, cap, nthreads=8)
    got = narrow_device(ctx, cfg, data, off, cap)
    for k in ("records8", "wide", "err_args", "flows"):
        assert got[k].tobytes() == nref[k].tobytes(), "%s/narrow: %s differs from the oracle" % (what, k)
    wide = np.nonzero(nref["records8"]["status"] & _lib.ST8_WIDE)[0]
    assert np.array_equal(np.nonzero(got["records8"]["status"] & _lib.ST8_WIDE)[0], wide), what
    w = check_equal(compact_device(ctx, cfg, data, off, cap, 64), nref, what + "/narrow compact")
    assert np.array_equal(w, wide), what
    seen.update((want, K_LAY, K_FIELDS))
    return ref, plain


def every_band(ctx, name, batch, what, check=None):
    """every_form in each band of the parser; a parser without an IPv6 decoder
    thereby goes through all five named kernels. check(ref, plain, band): the
    family's own assertions on the first len(batch) records."""
    from gopacket_amd import flows
    seen = set()
    grouper = flows.Grouper(8192)
    try:
        for band in BANDS_OF[name]:
            ref, plain = every_form(ctx, grouper, name, batch, band, "%s/%s/%s" % (what, name, band), seen)
            if check:
                check(ref, plain, band)
    finally:
        grouper.close()
    assert seen == (ALL_FIVE if name == "eth_ip4_tcp_payload" else {K_SB, K_BIG, K_LAY, K_FIELDS}), (what, name, seen)


def csum_count(ref, n):
    from gopacket_amd import _lib
    return int(((ref["records"]["status"][:n] & _lib.ST_L4_CSUM) != 0).sum())


@pytest.mark.parametrize("name", ["eth_ip4_tcp_payload", "statsassembly"])
@pytest.mark.parametrize("pattern", C.A_PATTERNS)
def test_saturated_wave(gpu_ctx, pattern, name):
    """Family A: 64 saturated frames (150 KiB: the dense prefix wraps 2^32 inside
    the wave) as one whole wave and across two, at all 16 byte phases."""
    for phases in C.A_PHASE_GROUPS:
        b, whole = C.family_a(pattern, phases)
        assert [b.offsets[w] % 16 for w in whole] == list(phases)

        def check(ref, plain, band, n=len(b)):
            assert csum_count(ref, n) == n
        every_band(gpu_ctx, name, b, "A/%s/phases %s" % (pattern, phases), check)


@pytest.mark.parametrize("name", ["eth_ip4_tcp_payload", "statsassembly", "raw_ip6"])
def test_residues_and_validity(gpu_ctx, name):
    """Family B: zero / saturated / alternating / single-bit payloads of 0..1025
    bytes under TCP and UDP over IPv4 and IPv6 at even and odd addresses, with
    the computed value steered to 0x0000, the field steered to valid, UDP's
    field 0, a field of 0xFFFF over zeros; saturated and 60-byte IPv4 headers,
    inside and across the header window."""
    from gopacket_amd import _lib
    b, labels = C.family_b(LINK_OF[name])

    def check(ref, plain, band):
        st = plain["records"]["status"][:len(b)]
        l4 = (st & _lib.ST_L4_CSUM) != 0
        assert l4.sum() >= (len(b) // 8 if name == "eth_ip4_tcp_payload" else len(b) // 2)
        assert (plain["records"]["l4_csum"][:len(b)][l4] == 0).sum() >= l4.sum() // 8  # the steered 0x0000 arrived
        assert 0 < ((st & _lib.ST_L4_VALID) != 0).sum() < l4.sum()
        if LINK_OF[name] == "eth":
            assert 0 < ((st & _lib.ST_IP4_VALID) != 0).sum() < ((st & _lib.ST_IP4_CSUM) != 0).sum()
    every_band(gpu_ctx, name, b, "B", check)


C_CASES = [("statsassembly", k) for k in C.C_KINDS["eth"]] + [("raw_ip6", k) for k in C.C_KINDS[None]] + \
          [("eth_ip4_tcp_payload", k) for k in ("tcp4", "x65536", "x65537")]


@pytest.mark.parametrize("name,kind", C_CASES)
def test_length_limits(gpu_ctx, name, kind):
    """Family C: saturated segments at the reachable maxima and on both sides of
    the 64 KiB rule (by the L4 segment and by the packet's extent), alone in a
    wave and with 63 packed neighbours, at even and odd addresses."""
    b, first = C.family_c(kind, LINK_OF[name])

    def check(ref, plain, band):
        assert csum_count(ref, len(b)) == 4 + 2 * 63
        col = plain["records"]["l4_csum"]
        assert len({int(col[i]) for i in first}) == 1  # one frame, four places
    every_band(gpu_ctx, name, b, "C/" + kind, check)


def test_uint32_wrap(gpu_ctx):
    """Family D: segments of 131 124 and 262 104 bytes of 0xFF, whose word sum
    wraps the reference's uint32: the device gives the reference's value, which
    is not the RFC 1071 one, at both start parities."""
    b, first = C.family_d()
    py = [C.py_checksums(b.packets[i], b.packets[i].layout(), "udp") for i in first[::2]]
    assert all(c.csum != c.csum_big for c in py)

    def check(ref, plain, band):
        assert csum_count(ref, len(b)) == len(b)
        got = [int(plain["records"]["l4_csum"][i]) for i in first]
        assert got == [py[0].csum, py[0].csum, py[1].csum, py[1].csum], (band, got, py)
    every_band(gpu_ctx, "raw_ip6", b, "D", check)


@pytest.mark.parametrize("name", ["eth_ip4_tcp_payload", "statsassembly"])
@pytest.mark.parametrize("ranges", ["segments", "extents"])
def test_predicate_boundary(gpu_ctx, ranges, name):
    """Family E: the same 64 saturated frames with the largest gap that keeps
    the wave dense, one byte more and 16 bytes more: the oracle's records each
    time, and the same checksums in all three waves."""
    b, g = C.family_e(ranges)

    def check(ref, plain, band):
        assert csum_count(ref, len(b)) == len(b)
        col = plain["records"]["l4_csum"]
        assert np.array_equal(col[:64], col[64:128]) and np.array_equal(col[:64], col[128:192])
    every_band(gpu_ctx, name, b, "E/%s (gap %d)" % (ranges, g), check)
