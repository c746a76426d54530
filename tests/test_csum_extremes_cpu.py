"""The checksum extremes of tests/csumcases.py, without a device: on every
packet whose status carries a checksum the oracle's ip4_csum, l4_csum and valid
bits equal csumcases.py_checksums, a second statement of the reference's
arithmetic in Python integers (this pins the oracle where the golden vectors do
not reach: saturated sums and the uint32 wrap of checksum.go:40-49), and every
case is what it claims to be: the saturated wave's prefix passes 2^32, the wrap
cases' RFC 1071 value differs from the reference's, the length pairs and the
boundary waves straddle dense_region's predicate, the steered packets compute
exactly the intended values."""
import numpy as np
import pytest

import csumcases as C
import pktutil
from configs import CONFIGS, oracle_parser
from gopacket_amd import _lib

PARSER_OF = {"eth": "statsassembly", None: "raw_ip6"}


def oracle_vs_py(name, batch, what, only=None):
    """The oracle's decode of the batch under parser `name`; every checksum it
    reports is compared with py_checksums (only: the packet indices to
    compare, default all). Returns (results, number of IPv4 sums compared, of L4 sums)."""
    data, off, cap = batch.finish()
    ref = oracle_parser(CONFIGS[name]).decode(data, off, cap, nthreads=4, layouts=True)
    rec, lay = ref["records"], ref["layouts"]
    n4 = nl4 = 0
    seen = {}
    for i in (range(len(batch)) if only is None else only):
        st = int(rec["status"][i])
        p = batch.packets[i]
        if st & _lib.ST_IP4_CSUM:
            c = C.py_checksums(p, lay[i], "ip4")
            assert (int(rec["ip4_csum"][i]), bool(st & _lib.ST_IP4_VALID)) == (c.csum, c.valid), (what, i, c)
            n4 += 1
        if st & _lib.ST_L4_CSUM:
            kind = "udp" if st & _lib.ST_L4_UDP else "tcp"
            key = (id(p), kind)  # the same frame object at another address: the same sums
            if key not in seen:
                seen[key] = C.py_checksums(p, lay[i], kind)
            c = seen[key]
            assert (int(rec["l4_csum"][i]), bool(st & _lib.ST_L4_VALID)) == (c.csum, c.valid), (what, i, c)
            assert c.csum != 0xFFFF, (what, i)  # needs a zero sum, which the protocol number rules out
            nl4 += 1
    l4 = (rec["status"] & _lib.ST_L4_CSUM) != 0
    assert not (rec["l4_csum"][l4] == 0xFFFF).any(), what
    return ref, n4, nl4


def test_builders_match_the_decode():
    """The jumbogram builder gives pktutil's packet for its payload, and the
    layer slices the builders claim are the oracle's, for every frame that
    decodes without an error (residues, headers, tags, limits)."""
    assert bytes(C.udp_jumbogram(b"\xfe" * 65536)) == pktutil.ipv6_udp_jumbogram(hbh16=True)
    batches = [(link, C.family_b(link)[0]) for link in ("eth", None)]
    batches += [(link, C.family_c(kind, link)[0]) for link in ("eth", None) for kind in C.C_KINDS[link]]
    for link, b in batches:
        data, off, cap = b.finish()
        ref = oracle_parser(CONFIGS[PARSER_OF[link]]).decode(data, off, cap, nthreads=4, layouts=True)
        ok = 0
        for i, p in enumerate(b.packets):
            if isinstance(p, C.Frame) and not int(ref["records"]["status"][i]) & _lib.ST_ERR_MASK:
                mine = p.layout()
                assert list(ref["layouts"]["start"][i]) == mine["start"], (link, i)
                assert list(ref["layouts"]["end"][i]) == mine["end"], (link, i)
                ok += 1
        assert ok >= len(b) // 2


def test_py_checksums_restates_the_fold_and_the_wrap():
    assert C.go_fold_checksum(0) == 0xFFFF and C.go_fold_checksum(0xFFFF) == 0 and C.go_fold_checksum(0x1FFFE) == 0
    assert C.go_compute_checksum(b"\xff\xff" * 70000, 0) == (0xFFFF * 70000) % (1 << 32)
    assert C.go_compute_checksum(b"\x01\x02\x03", 5) == 5 + 0x0102 + 0x0300
    with pytest.raises(AssertionError):
        f = C.frame("ip4", "tcp", b"ab")
        C.steer(f, f.payload, 0xFFFF)


@pytest.mark.parametrize("pattern", C.A_PATTERNS)
def test_saturated_wave(pattern):
    """Family A. The first phase pair against py_checksums; the other pairs hold
    the same packets at other addresses, so their records are the first pair's.
    For 0xFF payloads the whole wave's region L-sum passes 2^32 before its last
    segment starts, by the segments and by the packets' extents, and every wave
    is dense."""
    first = None
    for phases in C.A_PHASE_GROUPS:
        b, whole = C.family_a(pattern, phases)
        data, off, cap = b.finish()
        if first is None:
            ref, n4, nl4 = oracle_vs_py("statsassembly", b, "A/" + pattern)
            assert n4 == nl4 == len(b)
            first = ref["records"]
            valid = (first["status"] & _lib.ST_L4_VALID) != 0
            assert not valid[whole[0]:whole[0] + 64].any()  # a field of 0 / 0xFFFF is never the computed value here
        else:
            rec = oracle_parser(CONFIGS["statsassembly"]).decode(data, off, cap, nthreads=4, layouts=False)["records"]
            assert np.array_equal(rec, first), (pattern, phases)
        for ranges in ("segments", "extents"):
            plan = C.wave_plan(b.offsets, getattr(b, ranges)())
            assert all(w["dense"] and w["jobs"] == 64 for w in plan), (pattern, phases, ranges)
            for p, w0 in zip(phases, whole):
                assert w0 % 64 == 0 and b.offsets[w0] % 16 == p
                last = b.offsets[w0 + 63] + getattr(b, ranges)()[w0 + 63][0]
                lsum = C.region_lsum(data, plan[w0 // 64]["R0"], last)
                if pattern == "ff":
                    assert lsum > 1 << 32, (p, ranges, lsum)
                # two half-saturated waves follow, frames at lanes 32..63 and 0..31
                assert [len(x) for x in b.packets[w0 + 64:w0 + 192:32]] == [60, 2454, 2454, 60]
                assert b.offsets[w0 + 96] % 16 == p


def _label_checks(b, labels, ref):
    """The steered packets of family B compute exactly what their labels say."""
    rec, lay = ref["records"], ref["layouts"]
    counts = dict(computed0=0, valid=0, field0=0, fieldffff=0, twofold=0)
    for i, what in enumerate(labels):
        if what is None or what.startswith("winedge"):
            continue
        st = int(rec["status"][i])
        p = b.packets[i]
        hdr = what.startswith("ip4hdr")
        if hdr and not st & _lib.ST_IP4_CSUM:
            assert "all_ff" in what and st & _lib.ST_ERR_MASK, what  # the option's length exceeds the header
            continue
        assert st & (_lib.ST_IP4_CSUM if hdr else _lib.ST_L4_CSUM), what
        c = C.py_checksums(p, lay[i], "ip4" if hdr else p.kind)
        tag, where = what.rsplit("/", 1)[1].split("@")
        assert (b.offsets[i] + (p.l3 if hdr else p.l4)) % 2 == (where == "odd"), what
        if tag == "computed0":
            assert c.csum == 0 and c.field == 0 and (c.sum32 - c.field) % 65535 == 0
            assert c.valid  # a computed 0x0000 equals the field 0 (for UDP also valid by rule)
        elif tag == "computed0-field1234":
            assert c.csum == 0 and c.field == 0x1234 and (c.sum32 - c.field) % 65535 == 0
            assert not c.valid  # not even UDP: its rule needs a field of 0
        elif tag == "valid":
            assert c.valid and c.csum == c.field
        elif tag == "twofold":
            x = c.sum32 - c.field
            assert (x >> 16) + (x & 0xFFFF) > 0xFFFF and c.csum == ~(x >> 16) & 0xFFFF  # the fold's second iteration
        elif tag == "field0":
            assert c.field == 0 and c.valid == (c.csum == 0 or (p.kind == "udp" and not hdr))
        else:
            assert tag == "fieldffff" and c.field == 0xFFFF and not c.valid
            if not hdr:
                assert not any(p[p.payload:p.seg_end])
        counts["computed0" if tag.startswith("computed0") else tag] += 1
    return counts


@pytest.mark.parametrize("link", ["eth", None], ids=["eth", "raw"])
def test_residues_and_validity(link):
    """Family B against py_checksums, its labels, and the narrow form: exactly
    the packets whose checksums are not the fields' (or whose list is longer
    than 8) are widened."""
    b, labels = C.family_b(link)
    name = PARSER_OF[link]
    ref, n4, nl4 = oracle_vs_py(name, b, "B/%s" % name)
    counts = _label_checks(b, labels, ref)
    per = len(C.B_PATTERNS) * len(C.B_LENGTHS) * 2 * (2 if link == "eth" else 1) * 2  # both parities
    assert counts["valid"] >= per and counts["computed0"] >= 2 * per and counts["field0"] >= per
    assert counts["fieldffff"] >= per // len(C.B_PATTERNS) and counts["twofold"] >= per // 2
    rec = ref["records"]
    if link == "eth":
        # the option forms the oracle accepts: kind 0xFF / length 40 carries the header checksum, 40 x 0xFF does not
        for i, what in enumerate(labels):
            if what and what.startswith("ip4hdr"):
                assert bool(rec["status"][i] & _lib.ST_IP4_CSUM) == ("all_ff" not in what), what
        # the window-edge frames: valid saturated headers at every byte phase, 13..22 decoded layers
        edge = np.array([bool(w and w.startswith("winedge")) for w in labels])
        assert edge.sum() == 10 * 2 * 16
        assert (rec["status"][edge] & _lib.ST_IP4_VALID).all() and not (rec["status"][edge] & _lib.ST_ERR_MASK).any()
        # and the parser without IPv6 and UDP decoders still sums every IPv4 header and TCP segment
        ref2, m4, ml4 = oracle_vs_py("eth_ip4_tcp_payload", b, "B/eth_ip4_tcp_payload")
        assert m4 > 0 and ml4 > 0
    nar = oracle_parser(CONFIGS[name]).decode_narrow(*b.finish())
    wide = (nar["records8"]["status"] & _lib.ST8_WIDE) != 0
    st = rec["status"]
    nl = (st >> _lib.ST_NLAYERS_SHIFT) & _lib.ST_NLAYERS_MASK
    lay = ref["layouts"]
    want = nl > 8
    for i, p in enumerate(b.packets):
        if st[i] & _lib.ST_IP4_CSUM and rec["ip4_csum"][i] != C.py_checksums(p, lay[i], "ip4").field:
            want[i] = True
        if st[i] & _lib.ST_L4_CSUM and rec["l4_csum"][i] != C.py_checksums(p, lay[i], p.kind).field:
            want[i] = True
    assert np.array_equal(wide, want) and 0 < wide.sum() < len(wide)


C_PLAN = {  # kind: (dense by its L4 segment, dense by the packet's extent)
    "tcp4": (True, False), "tcp6": (True, False), "j65536": (True, False), "j65537": (False, False),
    "x65536": (True, True), "x65537": (True, False)}


@pytest.mark.parametrize("link,kind", [(l, k) for l in ("eth", None) for k in C.C_KINDS[l]],
                         ids=lambda v: v if v else "raw")
def test_length_limits(link, kind):
    """Family C against py_checksums; wave_plan says on which side of the
    64 KiB rule each frame lands, alone in its wave and with 63 neighbours; at
    these lengths the reference's uint32 does not wrap yet."""
    b, first = C.family_c(kind, link)
    assert [i % 64 for i in first] == [0] * 4 and [b.offsets[i] % 2 for i in first] == [0, 1, 0, 1]
    ref, n4, nl4 = oracle_vs_py(PARSER_OF[link], b, "C/%s" % kind, only=first + [first[2] + 1, first[3] + 63])
    assert nl4 == 6
    f = b.packets[first[0]]
    c = C.py_checksums(f, f.layout(), f.kind)
    assert c.sum_big == c.sum32 < 1 << 32 and c.csum == c.csum_big
    by_seg, by_ext = C.wave_plan(b.offsets, b.segments()), C.wave_plan(b.offsets, b.extents())
    assert [w["dense"] for w in by_seg] == [C_PLAN[kind][0]] * 4
    assert [w["dense"] for w in by_ext] == [C_PLAN[kind][1]] * 4
    assert [w["jobs"] for w in by_seg] == [1, 1, 64, 64] and [w["jobs"] for w in by_ext] == [64] * 4
    assert [w["far"] for w in by_seg] == [not C_PLAN[kind][0]] * 4  # the length rule, not the region's size


def test_uint32_wrap():
    """Family D: the segment's word sum passes 2^32, the reference's checksum
    (and the oracle's) is therefore not the RFC 1071 one, and both waves of
    each frame are sparse by the length rule."""
    b, first = C.family_d()
    ref, n4, nl4 = oracle_vs_py("raw_ip6", b, "D", only=first + [i + 1 for i in first])
    assert nl4 == 8
    for i, n in zip(first, (131124, 131124, 262104, 262104)):
        f = b.packets[i]
        assert f.seg_end - f.l4 == n
        c = C.py_checksums(f, ref["layouts"][i], "udp")
        assert c.sum_big >> 32 == 1 and c.sum32 == c.sum_big - (1 << 32)
        assert c.csum != c.csum_big and abs(c.csum - c.csum_big) == 1
        assert int(ref["records"]["l4_csum"][i]) == c.csum
    assert len(b.packets[first[2]]) == 262144
    assert [w["far"] for w in C.wave_plan(b.offsets, b.segments())] == [True] * 4
    assert [b.offsets[i] % 2 for i in first] == [0, 1, 0, 1]


@pytest.mark.parametrize("ranges", ["segments", "extents"])
def test_predicate_boundary(ranges):
    """Family E: at gap g the wave is dense, at g + 1 and g + 16 it is not, by
    the ranges named; the three waves hold the same packets, so the oracle gives
    them the same checksums."""
    b, g = C.family_e(ranges)
    assert len(b) == 192 and g > 100000
    plan = C.wave_plan(b.offsets, getattr(b, ranges)())
    assert [w["dense"] for w in plan] == [True, False, False] and not any(w["far"] for w in plan)
    assert plan[0]["R"] == 4 * plan[0]["tot"] + 8192 and plan[1]["R"] == plan[0]["R"] + 1
    ref, n4, nl4 = oracle_vs_py("statsassembly", b, "E/" + ranges, only=[0, 63, 64, 191])
    col = ref["records"]["l4_csum"]
    assert np.array_equal(col[:64], col[64:128]) and np.array_equal(col[:64], col[128:])
    assert ((ref["records"]["status"] & _lib.ST_L4_CSUM) != 0).all()
