"""gpk_tcpasm_batch (TCP reassembly in HBM, include/gpk_tcpasm.h) against the
reassembly model (tests/tcpasm_model.py) run on the decode oracle's results:
the same verdict and stream for every packet, the same streams in the same
order with the same chunks (every field), every byte of data, the same state
at the end (conn_seq, conn_stream, pending pages) and counts. No tolerance
anywhere."""
import ctypes
import functools

import numpy as np
import pytest

import flowcases
import pktutil
import tcpasm_model as M
import tcpasmcases as TC
from configs import device_parser, oracle_parser
from gopacket_amd import _lib, flows
from oracle import flows_oracle as FO

pytestmark = pytest.mark.gpu

CFG = flowcases.DEFRAG_PARSER
S, F, RST = TC.SYN, TC.FIN, TC.RST


def upload(packets):
    import torch
    data, off, cap = pktutil.pack(packets)
    n = len(packets)
    return (torch.from_numpy(data).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()[:n],
            torch.from_numpy(cap.astype(np.int32)).cuda()[:n])


def model(packets, **kw):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(CFG).decode(data, off, cap, layouts=True)
    return M.run(packets, res["records"], res["layouts"], **kw)


def device_assemble(gpu_ctx, packets, max_pages=0, flush=False, carry=(), chunk_cap=None, data_cap=None, guard=0):
    """-> host dict of every output array, cut to its used length"""
    import torch
    d, o, c = upload(packets)
    n = len(packets)
    m = max(n, 1)
    rec = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(3 * m, dtype=torch.int64, device="cuda")
    lay = torch.zeros(m * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(device_parser(CFG), d, o, c, rec, None, fl, lay, stream=torch.cuda.current_stream())
    g = flows.Grouper(m)
    asm = flows.Assembler(m)
    groups = g.group(d, o, c, rec, lay, kind=FO.CONNECTION)
    code = seq = None
    if carry:
        code = torch.tensor(np.array([k for k, _ in carry], np.uint32).view(np.int32), device="cuda")
        seq = torch.tensor([s for _, s in carry], dtype=torch.int64, device="cuda")
    out_data = None
    if data_cap is not None:
        out_data = torch.full((data_cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = asm.assemble(d, o, c, rec, lay, groups, max_pages=max_pages, flush=flush, chunk_cap=chunk_cap,
                       data_cap=data_cap, out_data=out_data, carry_code=code, carry_seq=seq)
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    G = int(groups["counts"][0].item())
    St, C, NP = counts[0], counts[1], counts[3]
    host = dict(counts=counts, G=G, verdict=out["verdict"].cpu().tolist(), stream_of=out["stream_of"].cpu().tolist(),
                data=out["data"].cpu().numpy(), chunks=out["chunks"].cpu().numpy().view(_lib.TCP_CHUNK_DTYPE),
                stream_group=out["stream_group"][:St].cpu().tolist(), stream_first=out["stream_first"][:St].cpu().tolist(),
                stream_closed=out["stream_closed"][:St].cpu().numpy().view(np.uint32).tolist(),
                stream_chunk0=out["stream_chunk0"][:St + 1].cpu().tolist(),
                stream_data0=out["stream_data0"][:St + 1].cpu().tolist(),
                conn_seq=out["conn_seq"][:G].cpu().tolist(), conn_stream=out["conn_stream"][:G].cpu().tolist(),
                pend_pkt=out["pend_pkt"].cpu().tolist(), pend_page=out["pend_page"].cpu().tolist())
    g.close()
    asm.close()
    return host


FIELDS = ("skip", "src", "src_off", "len", "call", "flags")


def compare(got, ref, chunk_cap=None, data_cap=None):
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got["verdict"], ref["verdict"])) if a != b]
    assert not bad and len(got["verdict"]) == len(ref["verdict"]), bad[:8]
    assert got["stream_of"] == ref["stream_of"]
    st = ref["streams"]
    want_counts = list(ref["counts"])
    C, D = want_counts[1], want_counts[2]
    if chunk_cap is not None:
        want_counts[5] = max(0, C - chunk_cap)
    if data_cap is not None:
        want_counts[6] = int(D > data_cap)
    assert got["counts"] == want_counts
    assert got["G"] == ref["groups"]
    assert got["stream_group"] == [s["group"] for s in st]
    assert got["stream_first"] == [s["first"] for s in st]
    assert got["stream_closed"] == [s["closed"] for s in st]
    assert got["stream_chunk0"] == [int(x) for x in np.cumsum([0] + [len(s["chunks"]) for s in st])]
    assert got["stream_data0"] == [int(x) for x in np.cumsum([0] + [len(s["data"]) for s in st])]
    assert got["conn_seq"] == ref["conn_seq"] and got["conn_stream"] == ref["conn_stream"]
    npend = len(ref["pend"]) if chunk_cap is None else min(len(ref["pend"]), chunk_cap)
    assert list(zip(got["pend_pkt"][:npend], got["pend_page"][:npend])) == ref["pend"][:npend]
    flat = [(j, ch) for j, s in enumerate(st) for ch in s["chunks"]]
    keep = len(flat) if chunk_cap is None else min(len(flat), chunk_cap)
    ch = got["chunks"][:keep]
    for f in FIELDS:
        want = np.array([c[f] for _, c in flat[:keep]], dtype=_lib.TCP_CHUNK_DTYPE[f])
        assert np.array_equal(ch[f], want), (f, np.flatnonzero(ch[f] != want)[:8])
    assert np.array_equal(ch["stream"], np.array([j for j, _ in flat[:keep]], np.uint32))
    dst, at = [], 0
    for s in st:
        for c in s["chunks"]:
            dst.append(at)
            at += c["len"]
    assert np.array_equal(ch["dst"], np.array(dst[:keep], np.uint64))
    blob, at = got["data"], 0
    for j, s in enumerate(st):
        end = at + len(s["data"])
        if data_cap is None or end <= data_cap:
            mine = blob[at:end].tobytes()
            assert mine == s["data"], ("stream", j, next(k for k in range(len(mine)) if mine[k] != s["data"][k]))
        at = end


def check(gpu_ctx, packets, **kw):
    ref = model(packets, **kw)
    got = device_assemble(gpu_ctx, packets, **kw)
    compare(got, ref)
    return ref, got


@pytest.mark.parametrize("name", sorted(TC.REFERENCE))
def test_reference_sequences(gpu_ctx, name):
    ref, got = check(gpu_ctx, TC.reference_packets(name), max_pages=4)
    assert got["counts"][0] == 1


RUNS = (1, 2, 63, 64, 65, 128, 129, 200)


def run_keys(rng, fin_inside):
    """One key per (run length, displacement): SYN, then `run` in-order
    segments; the last one moved to position 0, 63 or 64 of the key's packets
    (the lanes of the first 64-packet step and the first of the second), or a
    FIN on the middle segment."""
    pk, port = [], 1000
    for run in RUNS:
        for move in (None, 0, 63, 64):
            port += 1
            segs = TC.stream_segments(rng, int(rng.integers(0, 2 ** 32)), [int(x) for x in rng.integers(1, 1461, run)],
                                      fin=False, sport=port)
            if fin_inside:
                mid = 1 + run // 2
                segs[mid] = segs[mid][:14 + 20 + 13] + bytes([F | TC.ACK]) + segs[mid][14 + 20 + 14:]
            if move is not None:
                if move >= len(segs) - 1:
                    continue
                segs.insert(move, segs.pop())
            pk += segs
    return pk


@pytest.mark.parametrize("fin_inside", [False, True])
@pytest.mark.parametrize("flush", [False, True])
def test_runs_around_the_wave(gpu_ctx, fin_inside, flush):
    pk = run_keys(np.random.default_rng(17), fin_inside)
    ref, _ = check(gpu_ctx, pk, flush=flush)
    assert M.QUEUED in ref["verdict"] and ref["counts"][0] >= 20


@pytest.mark.parametrize("max_pages", [0, 300])
def test_large_keys(gpu_ctx, max_pages):
    """Keys of more than 256 pages (the list's LDS part): 700 segments, some of
    several pages, arriving reversed behind the SYN, so that every insert
    shifts the whole list and the list crosses from LDS into the key's slice;
    the same shuffled in windows; 600 in order (the in-order run in the large
    instantiation); and a list that empties and refills."""
    rng = np.random.default_rng(37)
    sizes = [int(x) for x in rng.choice([10, 700, 1460, 1900, 1901, 4000], 700)]
    a = TC.stream_segments(rng, 2 ** 32 - 40000, sizes, sport=4001)
    pk = [a[0]] + a[1:][::-1]
    b = TC.stream_segments(rng, 77, sizes, sport=4002)
    pk += [b[j] for j in sorted(range(len(b)), key=lambda j: j + 40 * rng.random())]
    pk += TC.stream_segments(rng, 5, [int(x) for x in rng.integers(1, 1461, 600)], sport=4003)
    c = TC.stream_segments(rng, 9, sizes[:300], sport=4004, fin=False)
    pk += [c[0]] + c[2:150][::-1] + [c[1]] + c[151:][::-1] + [c[150]]
    ref, _ = check(gpu_ctx, pk, max_pages=max_pages)
    assert ref["counts"][1] > 2000 and (max_pages or ref["counts"][3] == 0)
    ref, _ = check(gpu_ctx, pk[:-200], max_pages=max_pages)   # ends with a long list still pending
    assert ref["counts"][3] > 100
    check(gpu_ctx, pk, max_pages=max_pages, flush=True)


LENGTHS = (0, 1, 1899, 1900, 1901, 3800, 3801, 5700)


@pytest.mark.parametrize("max_pages", [0, 1, 2, 4])
def test_page_boundaries(gpu_ctx, max_pages):
    """Every payload length queued out of order behind a hole, on its own key;
    then one key with a three-page packet, a later packet that lands between
    two of its pages, and the segment that fills the hole."""
    rng = np.random.default_rng(23)
    pk = []
    for q, n in enumerate(LENGTHS):
        kw = dict(sport=2000 + q)
        flags = F if n == 0 else 0
        pk += [TC.seg(100, S, **kw), TC.seg(111 + n, 0, TC.body(rng, 30), **kw), TC.seg(111, flags, TC.body(rng, n), **kw),
               TC.seg(101, 0, TC.body(rng, 10), **kw)]
        kw = dict(sport=2100 + q)  # no SYN: everything waits; equal-seq pages
        pk += [TC.seg(500, flags, TC.body(rng, n), **kw), TC.seg(500, flags, TC.body(rng, n), **kw),
               TC.seg(400, 0, TC.body(rng, 50), **kw)]
    kw = dict(sport=2200)
    pk += [TC.seg(100, S, **kw), TC.seg(201, 0, TC.body(rng, 5700), **kw), TC.seg(201 + 2500, 0, TC.body(rng, 100), **kw),
           TC.seg(201 + 1900, 0, TC.body(rng, 7), **kw), TC.seg(101, 0, TC.body(rng, 100), **kw)]
    for flush in (False, True):
        ref, _ = check(gpu_ctx, pk, max_pages=max_pages, flush=flush)
    lists = [c["src_off"] for c in ref["streams"][-1]["chunks"]]
    assert 1900 in lists and 3800 in lists


ISNS = (0, 2 ** 30 - 1, 2 ** 30, 3 * 2 ** 30, 3 * 2 ** 30 + 1, 2 ** 32 - 1, 2 ** 32 - 10)


@pytest.mark.parametrize("max_pages", [0, 4])
def test_sequence_wrap(gpu_ctx, max_pages):
    rng = np.random.default_rng(29)
    pk = []
    for q, isn in enumerate(ISNS):
        for back in (0, 700, 2500):  # the stream starts at, or shortly before, the point
            base = (isn - back) % 2 ** 32
            sizes = [600, 1000, 1900, 50, 2000]
            for mode in range(3):
                kw = dict(sport=3000 + q * 16 + mode * 4 + (0 if not back else 1 if back == 700 else 2))
                segs = TC.stream_segments(rng, base, sizes, **kw)
                if mode == 1:  # reordered
                    segs = [segs[0], segs[3], segs[2], segs[5], segs[1], segs[4], segs[6]]
                if mode == 2:  # overlapping
                    segs.insert(3, TC.seg(base + 1 + 300, 0, TC.body(rng, 900), **kw))
                    segs.insert(2, TC.seg(base + 1 + 1500, 0, TC.body(rng, 2100), **kw))
                pk += segs
                kw["sport"] += 2000  # the same without the SYN
                pk += segs[1:]
    check(gpu_ctx, pk, max_pages=max_pages, flush=True)
    check(gpu_ctx, pk, max_pages=max_pages)


def test_quirks(gpu_ctx):
    a, b = dict(sport=10, dport=20), dict(src=TC.B4, dst=TC.A4, sport=20, dport=10)
    pk = [
        TC.seg(100, S, **a), TC.seg(100, S, **a),                         # retransmitted SYN
        TC.seg(101, 0, b"abcd", **a), TC.seg(101, 0, b"ab", **a),         # old retransmission: empty chunk
        TC.seg(103, 0, b"cdefgh", **a),                                   # overlap trimmed by byteSpan
        TC.seg(900, S | TC.ACK, **b), TC.seg(901, 0, b"reply", **b),      # the other direction: its own connection
        TC.seg(105, F, **a),                                              # End on an empty chunk
        TC.seg(109, 0, b"after fin", **a),                                # a new instance of the same key
        TC.seg(7, F, sport=11), TC.seg(8, RST, sport=11),                 # bare FIN / RST on an unknown key
        TC.seg(10, S, sport=12), TC.seg(13, F, b"cd", sport=12), TC.seg(15, 0, b"ef", sport=12),
        TC.seg(11, 0, b"ab", sport=12),                                   # End page not last in ret: stays open
        TC.seg(50, 0, b"mid", sport=13), TC.seg(60, 0, b"stream", sport=13),  # mid-stream start
        TC.seg(70, 0, b"x", sport=14), TC.seg(70, 0, b"y", sport=14), TC.seg(70, F, b"z", sport=14),  # equal seqs
        TC.seg(10, S | F, b"zz", sport=15),                               # the first SYN's chunk has no End
        TC.seg(0, S, sport=16), TC.seg(2 ** 31 + 5, 0, b"q", sport=16),   # Skip past 2^31
        TC.seg(20, S, v6=True, sport=17), TC.seg(21, F, b"six", v6=True, sport=17),
        TC.seg(20, S, vlan=3, sport=17), TC.seg(21, F, b"tagged", vlan=3, sport=17, pad=4),
    ]
    ref, got = check(gpu_ctx, pk)
    assert got["verdict"][9:11] == [M.NOCONN, M.NOCONN] and got["stream_of"][9:11] == [-1, -1]
    assert got["stream_of"][8] != got["stream_of"][0]
    ref, got = check(gpu_ctx, pk, flush=True)
    assert 2 ** 31 + 4 in got["chunks"]["skip"][:got["counts"][1]]
    check(gpu_ctx, pk, max_pages=1, flush=True)


def alignment_packets():
    """A mid-stream segment per key (flush delivers it as one chunk), placed
    behind a junk packet and a pad stream so that the source address and the
    destination offset take every pair of 16-byte phases; the lengths 0..70 and
    1899..1901 rotate over the pairs, so each meets many phases: the copy's
    paths depend on the head (-dst & 15), the source phase behind it, the
    number of 16-byte vectors and the tail."""
    rng = np.random.default_rng(31)
    lengths = list(range(0, 71)) + [1899, 1900, 1901]
    pk, at, done, port, pairs = [], 0, 0, 0, set()

    def add(p):
        nonlocal at
        pk.append(p)
        at += len(p)

    def key():
        nonlocal port
        port += 1
        return dict(sport=1 + port % 60000, dport=1 + port // 60000)

    for sp in range(16):
        for dp in range(16):
            for j in range(5):
                n = lengths[(sp * 16 + dp + 15 * j) % len(lengths)] or 0
                if n == 0:  # an empty payload needs a flag to be keyed
                    add(TC.seg(5, F, **key()))
                    continue
                pad = (dp - done) % 16
                if pad:
                    add(TC.seg(5, 0, TC.body(rng, pad), **key()))
                    done += pad
                junk = (sp - (at + 54)) % 16
                if junk:
                    add(b"\x01" * junk)
                assert (at + 54) % 16 == sp and done % 16 == dp
                add(TC.seg(5, 0, TC.body(rng, n), **key()))
                done += n
                if n >= 32:
                    pairs.add((sp, dp))
    assert len(pairs) == 256
    add(TC.seg(5, 0, TC.body(rng, 64000), **key()))  # many rounds of 64 vectors
    return pk


def test_copy_alignment(gpu_ctx):
    pk = alignment_packets()
    ref, got = check(gpu_ctx, pk, flush=True)
    assert ref["counts"][2] > 64000


@functools.lru_cache(maxsize=None)
def random_packets():
    return TC.random_traffic(7, 2500)


@pytest.mark.parametrize("max_pages,flush", [(0, False), (0, True), (4, False), (4, True)])
def test_random_traffic(gpu_ctx, max_pages, flush):
    pk = random_packets()
    ref, _ = check(gpu_ctx, pk, max_pages=max_pages, flush=flush)
    v = ref["verdict"]
    assert ref["counts"][0] > 2500 and M.QUEUED in v and M.NOCONN in v and FO.USELESS in v


def test_fuzz_packets_do_not_fault(gpu_ctx):
    pk = pktutil.fuzz_packets(91, 20000)
    ref, _ = check(gpu_ctx, pk, max_pages=4, flush=True)
    assert ref["counts"][0] > 0


def test_overflow(gpu_ctx):
    """chunk_cap and data_cap too small: the counts report the need, nothing is
    written past a cap (canaries behind every capped array), the streams that
    fit are whole and the others are not written at all."""
    import torch
    rng = np.random.default_rng(8)
    pk = []
    for q in range(6):
        pk += TC.stream_segments(rng, 1000 * q, [300 + q, 2500, 40], sport=50 + q)
    pk += [TC.seg(9, 0, b"wait", sport=99), TC.seg(19, 0, b"wait", sport=99)]
    ref = model(pk)
    sizes = [len(s["data"]) for s in ref["streams"]]
    C, need = ref["counts"][1], sum(sizes)
    dcap = sum(sizes[:3]) + 77  # ends inside the fourth stream
    got = device_assemble(gpu_ctx, pk, data_cap=dcap, guard=4096)
    compare(got, ref, data_cap=dcap)
    assert got["counts"][2] == need and got["counts"][6] == 1
    assert np.all(got["data"][sum(sizes[:3]):] == 0xA5)
    ccap = C - 5
    compare(device_assemble(gpu_ctx, pk, chunk_cap=ccap), ref, chunk_cap=ccap)
    # the C ABI with a cap of 1 and canaries behind the chunk and pending arrays
    d, o, c = upload(pk)
    n = len(pk)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(device_parser(CFG), d, o, c, rec, None, fl, lay, stream=torch.cuda.current_stream())
    g, asm = flows.Grouper(n), flows.Assembler(n)
    groups = g.group(d, o, c, rec, lay, kind=FO.CONNECTION)
    out = asm.assemble(d, o, c, rec, lay, groups)
    guard = 64
    chunks = torch.full(((1 + guard) * 40,), 0xA5, dtype=torch.uint8, device="cuda")
    pp = torch.full((1 + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pg = torch.full((1 + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    b = _lib.Batch(d.data_ptr(), o.data_ptr(), c.data_ptr(), n, d.numel())
    r = _lib.Results(rec.data_ptr(), None, None, lay.data_ptr())
    gs = _lib.Groups(*[groups[k].data_ptr() for k in ("group_of", "perm", "start", "first", "counts")])
    op = _lib.TcpasmOpts(0, 0, 0, None, None)
    st = _lib.TcpStreams(*[out[k].data_ptr() for k in ("verdict", "stream_of")], chunks.data_ptr(),
                         *[out[k].data_ptr() for k in ("stream_group", "stream_first", "stream_closed",
                                                       "stream_chunk0", "stream_data0", "conn_seq", "conn_stream")],
                         pp.data_ptr(), pg.data_ptr(), out["counts"].data_ptr(), out["data"].data_ptr(), 1,
                         out["data"].numel() - 16)
    _lib.check(_lib.lib().gpk_tcpasm_batch(asm.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(gs),
                                           ctypes.byref(op), ctypes.byref(st), None))
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    assert counts[:5] == ref["counts"][:5] and counts[5] == C - 1 and counts[3] == 2
    assert torch.all(chunks[40:] == 0xA5)
    assert pp[1:].eq(0x5A5A5A5A).all() and pg[1:].eq(0x5A5A5A5A).all()
    assert (int(pp[0]), int(pg[0])) == ref["pend"][0]
    first = chunks[:40].cpu().numpy().view(_lib.TCP_CHUNK_DTYPE)[0]
    assert int(first["src"]) == ref["streams"][0]["chunks"][0]["src"]
    g.close()
    asm.close()


def test_carried_entries(gpu_ctx):
    """Carried connections and pages, bad entries included; a batch of only
    carried entries with flush (a partly popped three-page packet among them)."""
    rng = np.random.default_rng(41)
    big = TC.seg(2101, 0, TC.body(rng, 5000), sport=70)
    pk = [TC.seg(100, S, sport=70), big, big, TC.seg(300, 0, b"other", sport=71), TC.seg(1, S, sport=72),
          TC.seg(400, 0, b"page without conn", sport=73), TC.seg(1, S, sport=70), big]
    carry = [(M.CARRY_CONN, 101), (M.CARRY_PAGE | 1, 0), (M.CARRY_PAGE | 2, 0), (M.CARRY_CONN, -1),
             (M.CARRY_CONN | M.CARRY_PAGE, 5), (M.CARRY_PAGE, 0), (M.CARRY_CONN, 7), (M.CARRY_PAGE | 3, 0)]
    for flush in (False, True):
        ref, got = check(gpu_ctx, pk, flush=flush, carry=carry)
    assert got["verdict"] == [M.CARRIED] * 4 + [M.EBADCARRY] * 4
    more = pk + [TC.seg(101, 0, TC.body(rng, 2000), sport=70), TC.seg(300, F, b"other", sport=71)]
    check(gpu_ctx, more, carry=carry, max_pages=2)
    check(gpu_ctx, more, carry=carry, flush=True)


def test_edges(gpu_ctx):
    import torch
    check(gpu_ctx, [flowcases.connection_cases()[2], b"\x00" * 10, flowcases.defrag_struct_cases()[0][1]])  # unkeyed
    check(gpu_ctx, [flowcases.connection_cases()[2]], flush=True)
    asm = flows.Assembler(4)
    z64, z32, z8 = (torch.zeros(1, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.uint8))
    groups = dict(group_of=z32, perm=z32, start=z32, first=z32, counts=torch.zeros(2, dtype=torch.int32, device="cuda"))
    out = asm.assemble(z8, z64[:0], z32[:0], z8, z8, groups, flush=True)
    torch.cuda.synchronize()
    assert out["counts"].cpu().tolist() == [0] * 8
    assert int(out["stream_chunk0"][0]) == 0 and int(out["stream_data0"][0]) == 0
    asm.close()


def test_shared_bytes_are_refused(gpu_ctx):
    """Ten packets that are the same 60 KB of data: the workspaces, sized from
    the data's size, cannot hold their pages. Nothing is assembled and
    counts[7] says so; the same packet once is fine."""
    import torch
    rng = np.random.default_rng(3)
    one = TC.seg(5, 0, TC.body(rng, 60000), sport=77)
    d, o, c = upload([one])
    o, c = o.repeat(10), c.repeat(10)
    rec = torch.zeros(10 * 16, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(30, dtype=torch.int64, device="cuda")
    lay = torch.zeros(10 * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(device_parser(CFG), d, o, c, rec, None, fl, lay, stream=torch.cuda.current_stream())
    g, asm = flows.Grouper(10), flows.Assembler(10)
    groups = g.group(d, o, c, rec, lay, kind=FO.CONNECTION)
    out = asm.assemble(d, o, c, rec, lay, groups, flush=True)
    torch.cuda.synchronize()
    assert out["counts"].cpu().tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert out["stream_of"].cpu().tolist() == [-1] * 10 and int(out["conn_seq"][0]) == M.NO_CONN
    out = asm.assemble(d, o[:1], c[:1], rec, lay, g.group(d, o[:1], c[:1], rec, lay, kind=FO.CONNECTION), flush=True)
    torch.cuda.synchronize()
    assert out["counts"].cpu().tolist() == [1, 32, 60000, 0, 0, 0, 0, 0]
    g.close()
    asm.close()


def stream_key(s):
    return [(c["src"], c["src_off"], c["len"], c["skip"], c["flags"]) for c in s["chunks"]]


def streaming_packets():
    rng = np.random.default_rng(53)
    pk = TC.random_traffic(11, 30, lo=2, hi=7)
    kw = dict(sport=9)
    pk[40:40] = [TC.seg(100, S, **kw), TC.seg(2201, 0, TC.body(rng, 5000), **kw)]
    pk[90:90] = [TC.seg(101, 0, TC.body(rng, 2100), **kw)]
    return pk


def run_streaming(gpu_ctx, pk, cuts, max_pages):
    """-> {global stream id: (chunk tuples with global src, bytes)} over the calls, flushed at the end"""
    import torch
    s = flows.TCPAssembler(gpu_ctx, device_parser(CFG), len(pk) + 64, max_pages=max_pages)
    acc, starts = {}, [0] + list(cuts)
    parts = [pk[a:b] for a, b in zip(starts, list(cuts) + [len(pk)])]
    results = []
    for part in parts:
        d, o, c = upload(part)
        results.append(s.assemble(d, o, c))
    results.append(s.flush_all())
    assert s.open_count == 0
    for res in results:
        blob = res["data"].cpu().numpy() if res["streams"] else None
        for st in res["streams"]:
            e = acc.setdefault(st["id"], ([], []))
            for ch in st["chunks"]:
                b, i = ch["src"]
                e[0].append((starts[b] + i, ch["src_off"], ch["len"], ch["skip"], ch["flags"]))
            e[1].append(blob[st["data0"]:st["data1"]].tobytes())
    s.close()
    return {k: (v[0], b"".join(v[1])) for k, v in acc.items()}


def test_streaming_every_cut(gpu_ctx):
    """A few hundred packets cut at every position into two calls, and at a
    dozen position pairs into three, each followed at the end by flush_all():
    per stream the same chunks and bytes as from one flushed batch. (Traffic
    leaves no multi-page packet partly popped between two calls, see
    test_tcpasm_cpu.test_carry_reproduces_the_state; the cuts do carry all the
    pages of the three-page packet of port 9 across a call.)"""
    pk = streaming_packets()
    assert 100 < len(pk) < 400
    for mp in (0, 2):
        whole = model(pk, max_pages=mp, flush=True)
        want = {j: (stream_key(s), s["data"]) for j, s in enumerate(whole["streams"])}
        cuts = [(c,) for c in range(0, len(pk) + 1, 1 if mp == 0 else 7)]
        cuts += [(a, a + 9 + a % 5) for a in range(3, len(pk) - 20, len(pk) // 12)]
        for cut in cuts:
            got = run_streaming(gpu_ctx, pk, cut, mp)
            assert got == want, (mp, cut)


def test_host_mirror_callback_order(gpu_ctx):
    """gopacket_amd.tcpassembly replays the device result as the reference's
    callbacks: the model's call log (New, Reassembled per call, ReassemblyComplete)
    in the same order with the same chunks, over three batches and FlushAll;
    FlushOlderThan and MaxBufferedPagesTotal name the scope decision."""
    from gopacket_amd import tcpassembly
    pk = streaming_packets()
    ref = model(pk, max_pages=3, flush=True)
    want, idx = [], {}
    for e in ref["log"]:
        if e[0] == "Reassembled":
            st = ref["streams"][e[1]]
            k = idx.get(e[1], 0)
            idx[e[1]] = k + e[3]
            at = sum(c["len"] for c in st["chunks"][:k])
            items = []
            for c in st["chunks"][k:k + e[3]]:
                items.append((st["data"][at:at + c["len"]], c["skip"], bool(c["flags"] & M.START),
                              bool(c["flags"] & M.END), float(c["src"])))
                at += c["len"]
            want.append(("Reassembled", e[1], items))
        else:
            want.append((e[0], e[1]))
    got = []

    class Stream(tcpassembly.Stream):
        def __init__(self, j):
            self.j = j

        def Reassembled(self, rs):
            got.append(("Reassembled", self.j, [(bytes(r.Bytes), r.Skip, r.Start, r.End, r.Seen) for r in rs]))

        def ReassemblyComplete(self):
            got.append(("ReassemblyComplete", self.j))

    class Factory(tcpassembly.StreamFactory):
        n = 0

        def New(self, net, transport):
            assert net.String().count("->") == 1 and transport.String().count("->") == 1
            got.append(("New", Factory.n))
            Factory.n += 1
            return Stream(Factory.n - 1)

    a = tcpassembly.NewAssembler(tcpassembly.NewStreamPool(Factory()), ctx=gpu_ctx, parser=device_parser(CFG),
                                 max_packets=1024)
    a.MaxBufferedPagesPerConnection = 3
    cuts = [0, 50, 97, len(pk)]
    for lo, hi in zip(cuts, cuts[1:]):
        data, off, cap = pktutil.pack(pk[lo:hi])
        a.AssembleBatch(data, off[:hi - lo], cap[:hi - lo], timestamps=[float(i) for i in range(lo, hi)])
    closed = a.FlushAll()
    # the model flushes the connections in stream order, as the mirror does
    assert got == want
    assert closed == sum(1 for e in ref["log"] if e[0] == "ReassemblyComplete" and e[2] & M.CALL_FLUSH)
    with pytest.raises(NotImplementedError, match="out of scope"):
        a.FlushOlderThan(0)
    a.MaxBufferedPagesTotal = 5
    with pytest.raises(NotImplementedError, match="MaxBufferedPagesTotal"):
        a.AssembleBatch(*pktutil.pack(pk[:2]))
    a.close()
