"""The batches of tests/streamwincases.py, without a device: every checksum the
oracle reports on them equals csumcases.py_checksums (the reference's
arithmetic restated in Python integers), the frames built valid are valid, and
every case is what it claims to be by streamwincases.wave_path, the Python
restatement of the big-packet kernel's stream-windows test and window
arithmetic: all 16 byte phases and all 64 start residues occur, windows end at
and cross a pass boundary, several windows own one granule, the batch edges
and the short last packet are where they should be, and the fallback waves
fall on the intended side of the wave-uniform test."""
import numpy as np
import pytest

import csumcases as C
import streamwincases as S
from configs import CONFIGS, oracle_parser
from gopacket_amd import _lib


def decode(case, name, layouts=True):
    return oracle_parser(CONFIGS[name]).decode(case.data, case.off, case.cap, nthreads=4, layouts=layouts)


_py = {}


def pin(case, name):
    """Every checksum of the oracle's decode against py_checksums; returns the results."""
    ref = decode(case, name)
    rec, lay = ref["records"], ref["layouts"]
    n4 = nl4 = 0
    for i, p in enumerate(case.packets):
        st = int(rec["status"][i])
        for kind, bit, vbit, col in (("ip4", _lib.ST_IP4_CSUM, _lib.ST_IP4_VALID, "ip4_csum"),
                                     ("l4", _lib.ST_L4_CSUM, _lib.ST_L4_VALID, "l4_csum")):
            if not st & bit:
                continue
            k = kind if kind == "ip4" else ("udp" if st & _lib.ST_L4_UDP else "tcp")
            key = (bytes(p), k, tuple(lay["start"][i]), tuple(lay["end"][i]))
            if key not in _py:
                _py[key] = C.py_checksums(p, lay[i], k)
            c = _py[key]
            assert (int(rec[col][i]), bool(st & vbit)) == (c.csum, c.valid), (case.name, name, i, kind, c)
            n4 += kind == "ip4"
            nl4 += kind == "l4"
    return ref, n4, nl4


def common(case):
    n = len(case.off)
    assert 1 <= n <= 1300 and len(case.packets) == n
    assert len(case.data) // n >= 1024, "the big-packet kernel needs a mean of 1 KiB"
    assert all(int(o) + int(c) <= len(case.data) for o, c in zip(case.off, case.cap))
    assert all(bytes(case.data[int(o):int(o) + int(c)]) == bytes(p) for o, c, p in zip(case.off, case.cap, case.packets))
    return S.wave_path(case.off, case.cap)


def test_wave_path_restates_the_window():
    assert S.window(0, 1500) == (0, 6) and S.window(15, 1500) == (0, 6) and S.window(16, 1500) == (16, 6)
    assert S.window(16, 0) == (16, 0) and S.window(5, 0) == (0, 1)
    assert S.window(5, 11) == (0, 1) and S.window(5, 12) == (0, 2)
    assert S.window(15, 80) == (0, 6) and S.window(0, 80) == (0, 5) and S.window(31, 2) == (16, 2)


def test_phases():
    case = S.case_phases()
    path = common(case)
    assert case.claims["first_phases"] == list(range(16))
    assert len(path) == 16 and all(w["stream"] for w in path)
    assert {int(o) & 15 for o in case.off} == set(range(16))
    assert all(p["cells"] == 6 for w in path for p in w["packets"])
    for name in case.parsers:
        ref, n4, nl4 = pin(case, name)
        assert n4 == nl4 == len(case.off)
        st = ref["records"]["status"]
        assert ((st & _lib.ST_L4_VALID) != 0).all() and ((st & _lib.ST_IP4_VALID) != 0).all()


def test_residues():
    case = S.case_residues()
    path = common(case)
    assert len(path) == 2 and [int(case.off[0]) & 15, int(case.off[64]) & 15] == [0, 5]
    for w in path:
        assert w["stream"]
        assert {p["residue"] for p in w["packets"]} == set(range(64))
        assert {p["residue"] for p in w["packets"] if p["crosses"]} == {59, 60, 61, 62, 63}
        assert [p["residue"] for p in w["packets"] if p["ends_at_edge"]] == [58]
    ref, n4, nl4 = pin(case, "statsassembly")
    assert n4 == nl4 == 128 and ((ref["records"]["status"] & _lib.ST_L4_VALID) != 0).all()


def test_owners():
    case = S.case_owners()
    path = common(case)
    assert len(path) == 4 and all(w["stream"] for w in path)
    cap = case.cap.reshape(4, 64)
    short = np.arange(64) % 8 != 7
    assert (cap[:, ~short] == 9000).all()
    assert cap[0, short].min() == 60 and cap[0, short].max() == 90
    assert (cap[1, short] < 16).all() and cap[1, short].min() == 1
    assert case.claims["zero"] == 2 * 64 + 20 and case.cap[case.claims["zero"]] == 0
    cells = np.array([[p["cells"] for p in w["packets"]] for w in path])
    # (no window byte: one cell of the bytes before it unless it starts a granule)
    assert path[2]["packets"][20]["cells"] == (1 if int(case.off[case.claims["zero"]]) & 15 else 0)
    assert set(cells[2, short]) >= {2, 3, 4, 5, 6} and (cells[1, short] <= 2).all()
    # windows that contain the same granule, and passes with several owners
    for w in (0, 3):
        pk = path[w]["packets"]
        assert sum(pk[q + 1]["h"] < pk[q]["h"] + pk[q]["cells"] for q in range(63)) >= 40
        starts = {}
        for p in pk:
            starts[p["h"] // 64] = starts.get(p["h"] // 64, 0) + 1
        assert max(starts.values()) >= 7
    ref, n4, nl4 = pin(case, "statsassembly")
    st = ref["records"]["status"].reshape(4, 64)
    assert ((st[:, ~short] & _lib.ST_L4_VALID) != 0).all() and ((st[0] & _lib.ST_L4_VALID) != 0).all()
    assert ((st[1, short] & _lib.ST_ERR_MASK) != 0).all()  # less than an Ethernet header
    bad = (np.arange(64) % 4 == 0) & short
    assert ((st[3, bad] & _lib.ST_L4_CSUM) != 0).all() and ((st[3, bad] & _lib.ST_L4_VALID) == 0).all()
    assert ((st[3, short & ~bad] & _lib.ST_L4_VALID) != 0).all()


@pytest.mark.parametrize("short_last", [False, True])
@pytest.mark.parametrize("n", S.EDGE_N)
def test_edges(n, short_last):
    case = S.case_edge(n, short_last)
    path = common(case)
    assert len(case.off) == n and len(path) == (n + 63) // 64 and all(w["stream"] for w in path)
    assert len(path[-1]["packets"]) == (n - 1) % 64 + 1
    last, w = path[-1]["packets"][-1], path[-1]
    if short_last:
        assert last["h"] + last["cells"] == (w["R"] + 15) // 16  # the window's last cell is the region's last granule
        assert case.cap[-1] == 20 and last["cells"] == 2 and int(case.off[-1]) & 15 == (3 + 1500 * (n - 1)) % 16
    ref, n4, nl4 = pin(case, "eth_ip4_tcp_payload")
    assert nl4 == n - short_last
    assert bool(ref["records"]["status"][-1] & (_lib.ST_ERR_MASK | _lib.ST_TRUNCATED)) == short_last


def test_fallback():
    case = S.case_fallback()
    path = dict(zip(S.FALLBACK_WAVES, common(case)))
    assert len(case.off) == 64 * len(S.FALLBACK_WAVES)
    want = dict(sorted=(True, True), reversed=(True, False), shuffled=(True, False), equal=(True, True),
                one_pair=(True, False), gap_inside=(True, True), gap_past=(False, True))
    for kind, w in path.items():
        assert (w["dense"], w["sorted"]) == want[kind], kind
        assert w["stream"] == (w["dense"] and w["sorted"])
    off = case.off.reshape(-1, 64).astype(np.int64)
    k = S.FALLBACK_WAVES.index
    assert (np.diff(off[k("reversed")]) < 0).all()
    assert (np.diff(off[k("one_pair")]) < 0).sum() == 1 and np.diff(off[k("one_pair")])[40] < 0
    assert (np.diff(off[k("equal")]) == 0).sum() == 48 and (np.diff(off[k("equal")]) >= 0).all()
    limit = 4 * 64 * 1500 + 8192
    assert path["gap_inside"]["R"] == limit and path["gap_past"]["R"] == limit + 1
    for name in case.parsers:
        ref, n4, nl4 = pin(case, name)
        assert nl4 == len(case.off) and ((ref["records"]["status"] & _lib.ST_L4_VALID) != 0).all()


def test_long_headers():
    case = S.case_long_headers()
    path = common(case)
    f = S.long_header_frame()
    assert (f.l3, f.l4, f.payload) == (22, 82, 142) and f.payload > 96
    assert len(path) == 2 and all(w["stream"] for w in path)
    cuts = set(int(c) for c in case.cap[64:] if c != 1500)
    for lo, hi in ((0, 14), (14, 18), (18, 22), (22, 42), (42, 82), (82, 102), (102, 142)):
        assert any(lo < c < hi for c in cuts), (lo, hi)
    assert {14, 18, 22, 42, 82, 102, 142} <= cuts | {18}  # and the boundaries themselves
    assert any(c < 96 for c in cuts) and any(c > 96 for c in cuts) and 96 in cuts
    ref, n4, nl4 = pin(case, "statsassembly")
    st = ref["records"]["status"]
    assert ((st[:64] & _lib.ST_L4_VALID) != 0).all() and ((st[:64] & _lib.ST_IP4_VALID) != 0).all()
    assert (ref["layouts"]["start"][0][[C.D1Q, C.IP4, C.TCP, C.PAY]] == [18, 22, 82, 142]).all()
    cut = case.cap[64:] != 1500
    inside = np.array([int(c) not in (14, 18, 22, 42, 82, 102) and c < 142 for c in case.cap[64:]])
    assert ((st[64:][cut & inside] & (_lib.ST_ERR_MASK | _lib.ST_TRUNCATED)) != 0).all()  # a header cut short
    assert ((st[64:][cut] & _lib.ST_L4_VALID) == 0).all() and ((st[64:][~cut] & _lib.ST_L4_VALID) != 0).all()


def test_the_narrow_forms_agree():
    """The narrow record of every case is the oracle's 16-byte record by the gpk_record8 rules."""
    for case in S.all_cases():
        for name in case.parsers:
            ref = decode(case, name, layouts=False)["records"]
            nar = oracle_parser(CONFIGS[name]).decode_narrow(case.data, case.off, case.cap, nthreads=4)
            wide = (nar["records8"]["status"] & _lib.ST8_WIDE) != 0
            assert np.array_equal(nar["wide"][wide], ref[wide]), (case.name, name)
            assert np.array_equal(nar["records8"]["layers"][~wide].astype(np.uint64), ref["layers"][~wide])
