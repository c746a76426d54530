"""Device == oracle, bit for bit (records, error arguments, flows), on the
batches of tests/streamwincases.py: the big-packet L4 kernel takes its header
windows out of the checksum stream, so the cases put windows at every byte
phase and at every granule of a pass (at and across the pass boundary), several
windows on one granule, windows of fewer than six cells, a caplen of 0, the
batch edges, waves that must load their windows instead (unsorted or not
packed), and headers longer than the window, whole and cut
(test_stream_windows_cpu.py pins the oracle on the same batches and asserts
that each is what it claims to be).

Every batch has a mean packet of at least 1 KiB and the launched kernel is
asserted by name; each runs through the 16-byte record with compact and with
global tables, the narrow record with its side array and the narrow record
with its compact list."""
import numpy as np
import pytest

import streamwincases as S
from configs import CONFIGS, assert_same, device_parser, oracle_parser
from test_gpu_parity import K_BIG
from test_narrow_compact_gpu import check_equal, compact_device
from test_narrow_gpu import narrow_device

pytestmark = pytest.mark.gpu


def every_form(ctx, case):
    from gopacket_amd import _lib
    data, off, cap = case.batch
    assert len(data) // len(off) >= 1024
    for name in case.parsers:
        what = "%s/%s" % (case.name, name)
        cfg = CONFIGS[name]
        dp, op = device_parser(cfg), oracle_parser(cfg)
        ref = op.decode(data, off, cap, nthreads=8, layouts=False)
        assert ctx.kernel_name(dp, data, off, cap, layouts=False) == K_BIG % "true", what
        assert_same(ctx.decode_host(dp, data, off, cap, layouts=False), ref, what + "/plain")
        ctx.set_table_mode(_lib.TABLES_GLOBAL)
        try:
            assert ctx.kernel_name(dp, data, off, cap, layouts=False) == K_BIG % "false", what
            assert_same(ctx.decode_host(dp, data, off, cap, layouts=False), ref, what + "/plain, global tables")
        finally:
            ctx.set_table_mode(_lib.TABLES_AUTO)
        nref = op.decode_narrow(data, off, cap, nthreads=8)
        got = narrow_device(ctx, cfg, data, off, cap)
        for k in ("records8", "wide", "err_args", "flows"):
            assert got[k].tobytes() == nref[k].tobytes(), "%s/narrow: %s differs from the oracle" % (what, k)
        check_equal(compact_device(ctx, cfg, data, off, cap, 64), nref, what + "/narrow compact")


def test_phases(gpu_ctx):
    every_form(gpu_ctx, S.case_phases())


def test_residues(gpu_ctx):
    every_form(gpu_ctx, S.case_residues())


def test_owners(gpu_ctx):
    every_form(gpu_ctx, S.case_owners())


@pytest.mark.parametrize("short_last", [False, True])
@pytest.mark.parametrize("n", S.EDGE_N)
def test_edges(gpu_ctx, n, short_last):
    every_form(gpu_ctx, S.case_edge(n, short_last))


def test_fallback(gpu_ctx):
    """The same 64 frames per wave in order, reversed, shuffled, named four
    times each, with one pair swapped and around the dense predicate: the
    oracle's records each time, and the same checksums whichever path a wave took."""
    case = S.case_fallback()
    every_form(gpu_ctx, case)
    rec = gpu_ctx.decode_host(device_parser(CONFIGS["statsassembly"]), *case.batch, layouts=False)["records"]
    col = rec["l4_csum"].reshape(-1, 64)
    k = S.FALLBACK_WAVES.index
    assert np.array_equal(col[k("sorted")], col[k("reversed")][::-1])
    assert np.array_equal(np.sort(col[k("sorted")]), np.sort(col[k("shuffled")]))
    assert np.array_equal(col[k("gap_inside")], col[k("gap_past")])


def test_long_headers(gpu_ctx):
    every_form(gpu_ctx, S.case_long_headers())
