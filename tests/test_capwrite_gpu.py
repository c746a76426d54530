"""gpk_capwrite_batch (the pcap / pcapng framing kernels, include/gpk_capwrite.h)
against the model (capwrite_model.py): every byte of out[:counts[1]],
block_off, status and counts, for the three formats and both group sizes of
the framing kernel (forced through gpk_capwrite_opts.group), on the shapes of
capwritecases.py: every capture length of 0..70 and 1490..1530 at every source
alignment and every output base offset, packets of 65 535 and 262 144 bytes,
m = 0, order NULL / a permutation / a selection with repeats / BPF.Select's
index, option blobs of 0, 4 and 40 bytes, both kinds of error packets, the
special timestamps, overflow at three cut points with a canary, and the
Python batch entry (WritePackets) with its first-error semantics. The device
output of a C4-mix batch is read back by the project's readers."""
import ctypes
import io

import numpy as np
import pytest

import bpfcases
import capwrite_model as M
import capwritecases as CC
from gopacket_amd import _lib, bpf, pcapgo as P, synth

pytestmark = pytest.mark.gpu

FORMATS = [M.PCAP_MICRO, M.PCAP_NANO, M.PCAPNG]
FILL = 0xA5


def upload(case):
    import torch
    return dict(d=torch.from_numpy(case["data"]).cuda(), o=torch.from_numpy(case["offsets"].astype(np.int64)).cuda(),
                c=torch.from_numpy(case["caplens"].astype(np.int32)).cuda(),
                ci=torch.from_numpy(case["ci"].view(np.uint8).copy()).cuda())


@pytest.fixture(scope="module")
def acase(gpu_ctx):
    case = CC.alignment_case()
    case["dev"] = upload(case)
    case["want"] = {}
    return case


def want(case, fmt, okind="none", order=None, blobs=False):
    """The model's result, computed once per (format, order, options)."""
    key = (fmt, okind, blobs)
    if key not in case["want"]:
        m = len(case["offsets"]) if order is None else len(order)
        case["want"][key] = CC.expected(fmt, case, order, CC.option_blobs(m) if blobs else None)
    return case["want"][key]


_writers = {}


def writer(fmt):
    if fmt not in _writers:
        L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(L.gpk_capwriter_create(ctypes.byref(h), fmt, 0, 8192))
        if fmt == M.PCAPNG:
            _lib.check(L.gpk_capwriter_set_interfaces(h, CC.INTERFACES))
        _writers[fmt] = h
    return _writers[fmt]


def run_device(fmt, case, order=None, blobs=None, out_cap=0, base=0, group=0):
    """One gpk_capwrite_batch into a buffer filled with FILL: out = buf + base,
    64 canary bytes and more after out_cap. Returns (buf, block_off, status, counts)."""
    import torch
    dev = case["dev"]
    n = len(case["offsets"])
    m = n if order is None else len(order)
    buf = torch.full((base + out_cap + 128,), FILL, dtype=torch.uint8, device="cuda")
    boff = torch.full((m + 1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((max(m, 1),), 99, dtype=torch.int32, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    od = oo = ot = None
    if blobs is not None:
        a, b = CC.pack_options(blobs)
        od, oo = torch.from_numpy(a).cuda(), torch.from_numpy(b.astype(np.int64)).cuda()
    if order is not None and m:
        ot = order if isinstance(order, torch.Tensor) else torch.from_numpy(order.astype(np.int32)).cuda()
    b = _lib.Batch(dev["d"].data_ptr(), dev["o"].data_ptr(), dev["c"].data_ptr(), n, dev["d"].numel())
    o = _lib.CapwriteOpts(CC.NOW[0], CC.NOW[1], group)
    _lib.check(_lib.lib().gpk_capwrite_batch(
        writer(fmt), ctypes.byref(b), ot.data_ptr() if ot is not None else None, m, dev["ci"].data_ptr(),
        od.data_ptr() if od is not None else None, oo.data_ptr() if oo is not None else None, ctypes.byref(o),
        buf.data_ptr() + base, out_cap, boff.data_ptr(), st.data_ptr(), cnt.data_ptr(),
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf.cpu().numpy(), boff.cpu().tolist(), st[:m].cpu().tolist(), cnt.cpu().tolist()


def check(res, expect, base, out_cap):
    buf, boff, st, cnt = res
    data, off, status, _ = expect
    fit = max(x for x in off if x <= out_cap)  # blocks are written while they end inside out_cap
    written = sum(1 for j, s in enumerate(status) if s == 0 and off[j + 1] <= out_cap)
    assert st == status and boff == off
    assert cnt == [written, off[-1], sum(1 for s in status if s), int(off[-1] > out_cap)]
    bad = np.flatnonzero(buf[base:base + fit] != np.frombuffer(data[:fit], np.uint8))
    assert len(bad) == 0, (bad[:8], np.searchsorted(off, bad[:8], side="right") - 1)
    assert (buf[:base] == FILL).all() and (buf[base + fit:] == FILL).all()


@pytest.mark.parametrize("group", [16, 64])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_length_and_alignment(acase, fmt, group):
    """1792 packets (112 lengths x 16 source alignments) at 16 output bases;
    options of 0 / 4 / 40 bytes and both error kinds mixed in."""
    exp = want(acase, fmt, blobs=True)
    n = len(acase["offsets"])
    assert exp[3][2] > 40 and (fmt != M.PCAPNG or {M.EIFACE, M.ELENGTH} <= set(exp[2]))
    for base in range(16):
        check(run_device(fmt, acase, None, CC.option_blobs(n), len(exp[0]), base, group), exp, base, len(exp[0]))


@pytest.mark.parametrize("group", [0, 16, 64])
@pytest.mark.parametrize("fmt", FORMATS)
def test_orders(acase, fmt, group):
    n = len(acase["offsets"])
    for okind, order in CC.orders(n).items():
        if order is None:
            continue
        exp = want(acase, fmt, okind, order)
        check(run_device(fmt, acase, order, None, len(exp[0]), 5, group), exp, 5, len(exp[0]))
    # BPF.Select's index, used as it comes from the device
    dev = acase["dev"]
    f = bpf.NewBPFInstructionFilter(bpfcases.PROGRAMS["len_gt_500_ret_a"])
    _, _, oi, k = f.Select(dev["d"], dev["o"], dev["c"])
    k = int(k.item())
    sel = np.flatnonzero(acase["caplens"] > 500).astype(np.uint32)
    assert k == len(sel) == 41 * 16 and np.array_equal(oi[:k].cpu().numpy(), sel)
    exp = want(acase, fmt, "select", sel)
    check(run_device(fmt, acase, oi[:k], None, len(exp[0]), 2, group), exp, 2, len(exp[0]))
    f.close()
    # an order entry that is no packet of the batch is an error packet, and m = 0 writes nothing
    order = np.array([3, n, 2000, 0xFFFFFFFF], np.uint32)
    exp = CC.expected(fmt, acase, order)
    assert exp[2][1] == exp[2][3] == M.EINDEX
    check(run_device(fmt, acase, order, None, len(exp[0]), 0, group), exp, 0, len(exp[0]))
    buf, boff, st, cnt = run_device(fmt, acase, np.zeros(0, np.uint32), None, 64, 0, group)
    assert boff == [0] and cnt == [0, 0, 0, 0] and (buf == FILL).all()


@pytest.mark.parametrize("group", [16, 64])
def test_big_packets(gpu_ctx, group):
    case = CC.big_case()
    case["dev"] = upload(case)
    for fmt in FORMATS:
        exp = CC.expected(fmt, case)
        for base in (0, 7):
            check(run_device(fmt, case, None, None, len(exp[0]), base, group), exp, base, len(exp[0]))


@pytest.mark.parametrize("group", [16, 64])
@pytest.mark.parametrize("fmt", [M.PCAP_MICRO, M.PCAPNG])
def test_overflow_writes_whole_blocks_only(acase, fmt, group):
    """out_cap inside a block, exactly at a block's end, and 0: the blocks
    before the cut as in the full run, nothing after them (the bytes of the
    unwritten blocks and the canary behind out_cap stay as they were)."""
    exp = want(acase, fmt, blobs=True)
    off = exp[1]
    n = len(acase["offsets"])
    for cut in (off[700] + 5, off[1200], 0):
        check(run_device(fmt, acase, None, CC.option_blobs(n), cut, 9, group), exp, 9, cut)


def device_batch(case):
    dev = case["dev"]
    return dev["d"], dev["o"], dev["c"]


def test_write_packets_stops_at_the_first_error(acase):
    import torch
    n = len(acase["offsets"])
    d, o, c = device_batch(acase)
    for fmt in FORMATS:
        blocks, off, status, counts = M.frame_batch(fmt, 1 if fmt == M.PCAPNG else 0, acase["packets"],
                                                    CC.ci_tuples(acase["ci"]), None, None, CC.NOW)
        b = io.BytesIO()
        if fmt == M.PCAPNG:
            w = P.NewNgWriter(b, 1)  # one interface: packets of interface 1 are in error too
        else:
            w = P.NewWriterNanos(b) if fmt == M.PCAP_NANO else P.NewWriter(b)
        head = len(b.getvalue())
        first = next(j for j, s in enumerate(status) if s)
        with pytest.raises(P.PcapgoError) as e:
            w.WritePackets(d, o, c, acase["ci"], now=CC.NOW)
        assert b.getvalue()[head:] == b"".join(blocks[:first])
        r = acase["ci"][first]
        if status[first] == M.EIFACE:
            assert e.value.text == "Can't send statistics for non existent interface %d; have only 1 interfaces" % \
                r["iface"]
        else:
            assert e.value.text == "invalid capture info {Timestamp:%s CaptureLength:%d Length:%d InterfaceIndex:%d " \
                "AncillaryData:[]}:  capture length > length" % (
                    P._go_time((int(r["ts_sec"]), int(r["ts_nsec"]))), acase["caplens"][first], r["length"], r["iface"])
        # skip_errors: everything else, through the device ci tensor and a selection
        b.seek(head)
        b.truncate()
        assert w.WritePackets(d, o, c, acase["dev"]["ci"], skip_errors=True, now=CC.NOW) == counts[0]
        assert b.getvalue()[head:] == b"".join(blocks)
        sel = np.arange(1, n, 3).astype(np.int32)
        b.seek(head)
        b.truncate()
        w.WritePackets(d, o, c, acase["ci"], order=torch.from_numpy(sel).cuda(), skip_errors=True, now=CC.NOW)
        assert b.getvalue()[head:] == b"".join(blocks[j] for j in sel)
        w.close()


def test_write_packets_with_options_and_repeats(acase):
    """NgPacketOptions per output packet, and an order with repeats whose
    blocks outgrow the first size estimate (the call is repeated)."""
    import torch
    d, o, c = device_batch(acase)
    order = np.array([1700, 1700, 1700, 40, 1700, 1791, 40], np.int32)
    opts = [None, P.NgPacketOptions(Comments=["c%d" % j for j in range(3)], Queue=7), None,
            P.NgPacketOptions(Flags=P.NgEpbFlags(Direction=1), DropCount=5, PacketID=1 << 60,
                              Hashes=[P.NgEpbHash(2, b"abcd")], Verdicts=[P.NgEpbVerdict(0, b"xyz")]), None, None,
            P.NgPacketOptions()]
    b = io.BytesIO()
    w = P.NewNgWriterInterface(b, P.DefaultNgInterface, P.DefaultNgWriterOptions)
    w.AddInterface(P.DefaultNgInterface)
    ci = acase["ci"].copy()
    ci["length"] = acase["caplens"]
    ci["iface"] %= 2
    ci["iface"] = np.abs(ci["iface"])
    assert w.WritePackets(d, o, c, ci, order=torch.from_numpy(order).cuda(), options=opts) == len(order)
    w.Flush()
    r = P.NewNgReader(b.getvalue())
    for j, i in enumerate(order):
        data, info, got = r.ReadPacketDataWithOptions()
        assert data == acase["packets"][i] and info.InterfaceIndex == ci["iface"][i]
        exp = opts[j] or P.NgPacketOptions()
        exp = P.NgPacketOptions(**{**exp.__dict__, "Comments": [x.encode() for x in exp.Comments]})
        assert got == exp, j
    with pytest.raises(EOFError):
        r.ReadPacketData()


def test_c4_mix_reads_back(gpu_ctx):
    """5 000 packets of the C4 IMIX mix written by the device in all three
    formats and read back by NgReader / Reader: the same packets and CaptureInfo."""
    import torch
    n = 5000
    d, o, c = synth.device_batch(synth.C4_IMIX, 17, n)
    hd, ho, hc = synth.host_batch(synth.C4_IMIX, 17, n)
    pk = [bytes(hd[a:a + k]) for a, k in zip(ho.tolist(), hc.tolist())]
    ci = np.zeros(n, _lib.CAPINFO_DTYPE)
    ci["ts_sec"] = 1600000000 + np.arange(n) // 7
    ci["ts_nsec"] = (np.arange(n) * 142857143) % 1000000000
    ci["length"] = hc + (np.arange(n) % 5 == 0) * 100
    ci["link_type"] = -1
    for fmt in FORMATS:
        b = io.BytesIO()
        if fmt == M.PCAPNG:
            w = P.NewNgWriter(b, P.LinkTypeEthernet)
        else:
            w = P.NewWriterNanos(b) if fmt == M.PCAP_NANO else P.NewWriter(b)
            w.WriteFileHeader(65536, P.LinkTypeEthernet)
        assert w.WritePackets(d, o, c, ci) == n
        r = P.NewNgReader(b.getvalue()) if fmt == M.PCAPNG else P.NewReader(b.getvalue())
        got = r.ReadBatch(n + 10)
        assert len(got) == n and np.array_equal(got.caplens, hc)
        assert [bytes(got.data[a:a + k]) for a, k in zip(got.offsets.tolist(), got.caplens.tolist())] == pk
        assert np.array_equal(got.ci["ts_sec"], ci["ts_sec"]) and np.array_equal(got.ci["length"], ci["length"])
        nsec = ci["ts_nsec"] // 1000 * 1000 if fmt == M.PCAP_MICRO else ci["ts_nsec"]
        assert np.array_equal(got.ci["ts_nsec"], nsec)
        with pytest.raises(EOFError):
            r.ReadPacketData()
        w.close()
    torch.cuda.synchronize()
