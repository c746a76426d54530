"""The capture writers on the CPU (include/gpk_capwrite.h, gopacket_amd.pcapgo):

- the checker (capwrite_model.py) against the reference's own byte vectors
  (tests/golden/capwrite_vectors.json, pcapgo/write_test.go:17-63) and, for
  pcapng, by round trip: the writer calls of TestNgWriteSimple
  (ngwrite_test.go:18-63), TestNgWriteComplex (:65-215),
  TestNgWritePacketWithOptions (:217-286) and TestNgWriterDSB
  (ngwrite_dsb_test.go) restated, the model's bytes read back with the
  project's NgReader, and sections, interfaces, statistics, packets,
  CaptureInfo and options compared with what the reference's tests expect;
- the Python mirror (NewWriter, NewNgWriter, ...) making the same calls into an
  io.BytesIO: the same bytes as the model;
- TestCaptureInfoErrors (write_test.go:82-103);
- the host block builders and gpk_capwrite_batch_host against the model, byte
  for byte, on the case generator the device test uses;
- the new structs' layouts against the C compiler's.
No GPU call is made here."""
import ctypes
import dataclasses
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import capwrite_model as M
import capwritecases as CC
from gopacket_amd import _lib, pcapgo as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VEC = json.load(open(os.path.join(GOLD, "capwrite_vectors.json")))
SRC = [bytes.fromhex(h) for h in json.load(open(os.path.join(GOLD, "pcapgo", "expect.json")))["ngPacketSource"]]
T0 = 1519128000
FRAC = 195312500


# ---- the reference's pcap vectors
def test_model_equals_reference_vectors():
    for h in VEC["headers"]:
        w = M.PcapWriter(nanos=h["nanos"])
        w.write_file_header(h["snaplen"], h["linktype"])
        assert bytes(w.out).hex() == h["want"], h["test"]
    p = VEC["packet"]
    w = M.PcapWriter(nanos=p["nanos"])
    w.write_packet((p["ts_sec"], p["ts_nsec"]), p["capture_length"], p["length"], bytes.fromhex(p["data"]))
    assert bytes(w.out).hex() == p["want"]


def test_mirror_equals_reference_vectors():
    for h in VEC["headers"]:
        b = io.BytesIO()
        (P.NewWriterNanos if h["nanos"] else P.NewWriter)(b).WriteFileHeader(h["snaplen"], h["linktype"])
        assert b.getvalue().hex() == h["want"], h["test"]
    p = VEC["packet"]
    b = io.BytesIO()
    P.NewWriter(b).WritePacket(P.CaptureInfo((p["ts_sec"], p["ts_nsec"]), p["capture_length"], p["length"]),
                               bytes.fromhex(p["data"]))
    assert b.getvalue().hex() == p["want"]


def test_capture_info_errors():  # TestCaptureInfoErrors
    data = bytes([1, 2, 3, 4])
    for length, caplen, text in ((5, 5, "capture length 5 does not match data length 4"),
                                 (3, 4, "invalid capture info {Timestamp:1970-01-01 00:00:00 +0000 UTC "
                                        "CaptureLength:4 Length:3 InterfaceIndex:0 AncillaryData:[]}:  "
                                        "capture length > length")):
        b = io.BytesIO()
        with pytest.raises(P.PcapgoError) as e:
            P.NewWriter(b).WritePacket(P.CaptureInfo((0, 0), caplen, length), data)
        assert e.value.text == text and b.getvalue() == b""
        with pytest.raises(M.WriteError):
            M.PcapWriter().write_packet((0, 0), caplen, length, data)
        with pytest.raises(P.PcapgoError):
            P.NewNgWriter(io.BytesIO(), 1).WritePacket(P.CaptureInfo((0, 0), caplen, length), data)


# ---- the reference's pcapng writer tests, restated for the model and the mirror
DEFAULT_SECTION = dict(Hardware=b"amd64", OS=b"linux", Application=b"gopacket")
DEFAULT_INTF = dict(Name=b"intf0", OS=b"linux", LinkType=1)


def read_back(raw):
    r = P.NewNgReader(raw)
    packets = []
    while True:
        try:
            packets.append(r.ReadPacketDataWithOptions())
        except EOFError:
            break
    return r, packets


def mirror_intf(**kw):
    return dataclasses.replace(P.DefaultNgInterface, **dict(dict(OS=b"", Name=b""), **kw))


def ng_simple():
    ci = ((0, 0), len(SRC[0]), len(SRC[0]), 0)
    m = M.NgWriter(DEFAULT_INTF, DEFAULT_SECTION)
    m.write_packet(ci[0], ci[1], ci[2], ci[3], SRC[0])
    b = io.BytesIO()
    w = P.NewNgWriter(b, P.LinkTypeEthernet)
    w.WritePacket(P.CaptureInfo(*ci), SRC[0])
    w.Flush()
    return bytes(m.out), b.getvalue()


def test_ng_write_simple():
    raw, mirrored = ng_simple()
    assert mirrored == raw
    r, packets = read_back(raw)
    assert r.LinkType() == P.LinkTypeEthernet and r.NInterfaces() == 1
    assert r.SectionInfo() == P.DefaultNgWriterOptions.SectionInfo
    want = dataclasses.replace(P.DefaultNgInterface, LinkType=P.LinkTypeEthernet)
    got = r.Interface(0)
    assert dataclasses.replace(got, Statistics=want.Statistics) == want
    assert [(d, ci.Timestamp, ci.CaptureLength, ci.Length, ci.InterfaceIndex) for d, ci, _ in packets] == \
        [(SRC[0], (0, 0), len(SRC[0]), len(SRC[0]), 0)]


COMPLEX_PACKETS = [  # (data, seconds before T0, wire length, interface)
    (SRC[0], 900, len(SRC[0]), 0), (SRC[4], 800, len(SRC[4]), 1), (SRC[1], 500, len(SRC[1]), 0),
    (SRC[2][:96], 300, len(SRC[2]), 0), (SRC[3], 200, len(SRC[3]), 0)]
STATS0 = dict(LastUpdate=(T0, FRAC), StartTime=(T0 - 100, FRAC), EndTime=(T0, FRAC), PacketsReceived=100,
              PacketsDropped=1)
STATS1 = dict(LastUpdate=(T0, FRAC), StartTime=M.ZERO, EndTime=M.ZERO, PacketsReceived=0, PacketsDropped=0)


def ng_complex():
    i0 = dict(Name=b"in0", Comment=b"test0", Description=b"some test interface", LinkType=1)
    i1 = dict(Name=b"null0", Description=b"some test interface", Filter=b"none", OS=b"not needed", LinkType=1,
              TimestampOffset=100)
    m = M.NgWriter(i0, dict(Comment=b"A test"))
    b = io.BytesIO()
    w = P.NewNgWriterInterface(b, mirror_intf(Name="in0", Comment="test0", Description="some test interface",
                                              LinkType=1, TimestampResolution=3),
                               P.NgWriterOptions(P.NgSectionInfo(b"", b"", b"", b"A test")))

    def packet(k):
        d, ago, length, iface = COMPLEX_PACKETS[k]
        m.write_packet((T0 - ago, FRAC), len(d), length, iface, d)
        w.WritePacket(P.CaptureInfo((T0 - ago, FRAC), len(d), length, iface), d)

    def stats(i, s):
        m.write_interface_stats(i, s)
        w.WriteInterfaceStats(i, P.NgInterfaceStatistics(s["LastUpdate"], s["StartTime"], s["EndTime"], b"",
                                                         s["PacketsReceived"], s["PacketsDropped"]))

    packet(0)
    assert m.add_interface(i1) == 1
    assert w.AddInterface(mirror_intf(Name="null0", Description="some test interface", Filter="none",
                                      OS="not needed", LinkType=1, TimestampOffset=100)) == 1
    packet(1)
    stats(1, STATS1)
    packet(2)
    packet(3)
    packet(4)
    stats(0, STATS0)
    w.Flush()
    return bytes(m.out), b.getvalue()


def test_ng_write_complex():
    raw, mirrored = ng_complex()
    assert mirrored == raw
    r, packets = read_back(raw)
    assert r.SectionInfo() == P.NgSectionInfo(b"", b"", b"", b"A test")
    assert r.NInterfaces() == 2 and r.LinkType() == 1
    # the writer fixes the resolution to 9; the reader adds interface 1's offset of 100 s
    assert r.Interface(0) == P.NgInterface(
        b"in0", b"test0", b"some test interface", b"", b"", 1, 9, 0, 0,
        P.NgInterfaceStatistics((T0, FRAC), (T0 - 100, FRAC), (T0, FRAC), b"", 100, 1))
    assert r.Interface(1) == P.NgInterface(
        b"null0", b"", b"some test interface", b"none", b"not needed", 1, 9, 100, 0,
        P.NgInterfaceStatistics((T0 + 100, FRAC), M.ZERO, M.ZERO, b"", 0, 0))
    want = [(d, (T0 - ago + (100 if iface else 0), FRAC), len(d), length, iface)
            for d, ago, length, iface in COMPLEX_PACKETS]
    assert [(d, ci.Timestamp, ci.CaptureLength, ci.Length, ci.InterfaceIndex) for d, ci, _ in packets] == want


MD5 = bytes.fromhex("900150983cd24fb0d6963f7d28e17f72")
LLERR = 0xFF000000  # symbol | preamble | SFD | unaligned | IFG | too short | too long | CRC


def test_ng_write_packet_with_options():
    flags = P.NgEpbFlags(Direction=0b01, Reception=0b01100, FCSLen=(10 << 5) & 0b1111100000, LinkLayerErr=LLERR)
    opts = P.NgPacketOptions(
        Comments=["this is a comment", "foobar"], Flags=flags,
        Hashes=[P.NgEpbHash(3, MD5), P.NgEpbHash(2, MD5[:4])], DropCount=2, PacketID=0x1234567890abcdef, Queue=1,
        Verdicts=[P.NgEpbVerdict(2, bytes(7) + b"\x01"), P.NgEpbVerdict(1, bytes(7) + b"\x02")])
    m = M.NgWriter(DEFAULT_INTF, DEFAULT_SECTION)
    m.write_packet((0, 0), len(SRC[0]), len(SRC[0]), 0, SRC[0], dict(
        Comments=[b"this is a comment", b"foobar"], Flags=flags.ToUint32(), Hashes=[(3, MD5), (2, MD5[:4])],
        DropCount=2, PacketID=0x1234567890abcdef, Queue=1,
        Verdicts=[(2, bytes(7) + b"\x01"), (1, bytes(7) + b"\x02")]))
    b = io.BytesIO()
    w = P.NewNgWriter(b, P.LinkTypeEthernet)
    w.WritePacketWithOptions(P.CaptureInfo((0, 0), len(SRC[0]), len(SRC[0])), SRC[0], opts)
    w.Flush()
    assert b.getvalue() == bytes(m.out)
    _, packets = read_back(bytes(m.out))
    assert len(packets) == 1
    d, ci, got = packets[0]
    assert d == SRC[0] and ci.Timestamp == (0, 0)
    assert got == dataclasses.replace(opts, Comments=[b"this is a comment", b"foobar"])
    assert flags.ToUint32() == 0xFF00014D


def test_ng_writer_dsb():  # TestNgWriterDSB / createPcapng, and ErrUnknownSecretsType
    key = (b"CLIENT_RANDOM 65bafa1a1a37aebce6ab7af420f9a6ca10513ad1d53aececbe831a28982a5c18 8d1e0c21e653f8e0720c987c3"
           b"daaca094ff6eb1ccc9e15a8384a214139dfdcf25f0ee77ac81250c7a11b8da561313528\n")
    sec = dict(Hardware=b"eCapture Hardware", Application=b"ecapture.lua",
               Comment=b"see https://ecapture.cc for more information.")
    i0 = dict(Name=b"eth0", Comment=b"gopacket: https://github.com/google/gopacket", LinkType=1, SnapLength=0xFFFF)
    m = M.NgWriter(i0, sec)
    b = io.BytesIO()
    w = P.NewNgWriterInterface(b, mirror_intf(Name="eth0", Comment="gopacket: https://github.com/google/gopacket",
                                              LinkType=1, SnapLength=0xFFFF),
                               P.NgWriterOptions(P.NgSectionInfo(sec["Hardware"], b"", sec["Application"],
                                                                 sec["Comment"])))
    for name in (b"lo", b"eth1"):
        m.add_interface(dict(Name=name, Comment=sec["Comment"], LinkType=1, SnapLength=0xFFFF))
        w.AddInterface(mirror_intf(Name=name, Comment=sec["Comment"], LinkType=1, SnapLength=0xFFFF))
    for payload in (key, b"", b"abcde"):
        m.write_secrets(M.SECRET_TYPES[4], payload)
        w.WriteDecryptionSecretsBlock(P.DSB_SECRETS_TYPE_TLS, payload)
    for k, d in enumerate(SRC):
        m.write_packet((T0 + k, k), len(d), len(d), k % 3, d)
        w.WritePacket(P.CaptureInfo((T0 + k, k), len(d), len(d), k % 3), d)
    assert b.getvalue() == bytes(m.out)
    with pytest.raises(P.PcapgoError) as e:
        w.WriteDecryptionSecretsBlock(0x12345678, b"x")
    assert e.value.text == "Unknown Decryption Secrets Block (DSB) type"
    with pytest.raises(M.WriteError):
        m.write_secrets(0x12345678, b"x")
    assert b.getvalue() == bytes(m.out)
    r, packets = read_back(bytes(m.out))
    assert r.SectionInfo() == P.NgSectionInfo(sec["Hardware"], b"", sec["Application"], sec["Comment"])
    assert r.NInterfaces() == 3 and r.Interface(2).Name == b"eth1" and r.Interface(0).SnapLength == 0xFFFF
    assert [(d, ci.Timestamp, ci.InterfaceIndex) for d, ci, _ in packets] == \
        [(d, (T0 + k, k), k % 3) for k, d in enumerate(SRC)]


def test_interface_errors_and_counts():
    b = io.BytesIO()
    w = P.NewNgWriter(b, 1)
    size = len(b.getvalue())
    for bad in (1, -1):
        with pytest.raises(P.PcapgoError) as e:
            w.WriteInterfaceStats(bad, P.ngEmptyStatistics)
        assert e.value.text == "Can't send statistics for non existent interface %d; have only 1 interfaces" % bad
        with pytest.raises(P.PcapgoError) as e:  # the interface is checked before the lengths (ngwrite.go:362-370)
            w.WritePacket(P.CaptureInfo((0, 0), 9, 3, bad), b"1234")
        assert e.value.text == "Can't send statistics for non existent interface %d; have only 1 interfaces" % bad
    assert len(b.getvalue()) == size
    m = M.NgWriter(DEFAULT_INTF, DEFAULT_SECTION)
    with pytest.raises(M.WriteError):
        m.write_interface_stats(1, {})
    # empty statistics: no option, no end-of-options
    w.WriteInterfaceStats(0, P.ngEmptyStatistics)
    m.write_interface_stats(0, {})
    assert b.getvalue() == bytes(m.out) and len(m.out) - size == 24
    # an interface with every string empty still carries if_tsresol, written as 4 bytes
    w.AddInterface(mirror_intf(LinkType=0))
    m.add_interface({})
    assert b.getvalue() == bytes(m.out) and bytes(m.out[-16:-8]) == b"\x09\x00\x01\x00\x09\x00\x00\x00"
    # a filter carries its leading 0 byte; odd string lengths are padded
    w.AddInterface(mirror_intf(Filter="tcp", Name="abcde", LinkType=1, TimestampOffset=1 << 40))
    m.add_interface(dict(Filter=b"tcp", Name=b"abcde", LinkType=1, TimestampOffset=1 << 40))
    assert b.getvalue() == bytes(m.out) and b"\x0b\x00\x04\x00\x00tcp" in bytes(m.out)


def test_pcap_zero_time_takes_now_and_nanos():
    for nanos in (False, True):
        m = M.PcapWriter(nanos=nanos, now=CC.NOW)
        b = io.BytesIO()
        w = P.NewWriterNanos(b) if nanos else P.NewWriter(b)
        for ts in CC.TIMES:
            m.write_packet(ts, 3, 4, b"abc")
            w.WritePacket(P.CaptureInfo(ts, 3, 4), b"abc", now=CC.NOW)
        assert b.getvalue() == bytes(m.out)


# ---- gpk_capwrite_batch_host against the model
def host_writer(fmt):
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.gpk_capwriter_create(ctypes.byref(h), fmt, -1, 0))
    if fmt == M.PCAPNG:
        _lib.check(L.gpk_capwriter_set_interfaces(h, CC.INTERFACES))
        assert L.gpk_capwriter_interfaces(h) == CC.INTERFACES
    return h


def run_host(fmt, case, order=None, blobs=None, out_cap=None, base=0):
    L = _lib.lib()
    h = host_writer(fmt)
    m = len(case["offsets"]) if order is None else len(order)
    want, off, _, _ = CC.expected(fmt, case, order, blobs)
    cap = len(want) if out_cap is None else out_cap
    buf = np.full(base + cap + 64, 0xA5, np.uint8)
    boff, st, cnt = np.zeros(m + 1, np.uint64), np.zeros(max(m, 1), np.int32), np.zeros(4, np.uint64)
    od = oo = None
    if blobs is not None:
        od, oo = CC.pack_options(blobs)
    b = _lib.Batch(case["data"].ctypes.data, case["offsets"].ctypes.data, case["caplens"].ctypes.data,
                   len(case["offsets"]), len(case["data"]))
    o = _lib.CapwriteOpts(CC.NOW[0], CC.NOW[1], 0)
    _lib.check(L.gpk_capwrite_batch_host(
        h, ctypes.byref(b), order.ctypes.data if order is not None else None, m, case["ci"].ctypes.data,
        od.ctypes.data if od is not None else None, oo.ctypes.data if oo is not None else None, ctypes.byref(o),
        buf.ctypes.data + base, cap, boff.ctypes.data, st.ctypes.data, cnt.ctypes.data))
    L.gpk_capwriter_destroy(h)
    return buf, boff.tolist(), st[:m].tolist(), cnt.tolist()


@pytest.fixture(scope="module")
def acase():
    return CC.alignment_case()


@pytest.mark.parametrize("fmt", [M.PCAP_MICRO, M.PCAP_NANO, M.PCAPNG])
@pytest.mark.parametrize("okind", ["none", "permutation", "repeats"])
def test_batch_host_equals_model(acase, fmt, okind):
    order = CC.orders(len(acase["offsets"]))[okind]
    m = len(acase["offsets"]) if order is None else len(order)
    blobs = CC.option_blobs(m)
    want, off, status, counts = CC.expected(fmt, acase, order, blobs)
    buf, boff, st, cnt = run_host(fmt, acase, order, blobs, base=3)
    assert st == status and boff == off and cnt == counts
    assert buf[3:3 + len(want)].tobytes() == want
    assert (buf[:3] == 0xA5).all() and (buf[3 + len(want):] == 0xA5).all()
    assert counts[2] > 10 and (fmt != M.PCAPNG or {M.EIFACE, M.ELENGTH} <= set(status))


@pytest.mark.parametrize("fmt", [M.PCAP_MICRO, M.PCAPNG])
def test_batch_host_overflow_and_edges(acase, fmt):
    want, off, status, counts = CC.expected(fmt, acase)
    for cut in (off[700] + 5, off[1200], 0):
        _, _, _, wc = CC.expected(fmt, acase, out_cap=cut)
        buf, boff, st, cnt = run_host(fmt, acase, out_cap=cut)
        assert boff == off and st == status and cnt == wc and cnt[3] == 1 and cnt[1] == len(want)
        fit = max(o for o in off if o <= cut)
        assert buf[:fit].tobytes() == want[:fit] and (buf[fit:] == 0xA5).all()
    # m = 0, and an order entry that is no packet of the batch
    buf, boff, st, cnt = run_host(fmt, acase, order=np.zeros(0, np.uint32))
    assert boff == [0] and cnt == [0, 0, 0, 0]
    order = np.array([1, len(acase["offsets"]), 2], np.uint32)
    want3, off3, status3, counts3 = CC.expected(fmt, acase, order)
    buf, boff, st, cnt = run_host(fmt, acase, order)
    assert st == status3 == [0, M.EINDEX, 0] and boff == off3 and cnt == counts3
    assert buf[:len(want3)].tobytes() == want3


def test_batch_host_big_packets():
    case = CC.big_case()
    for fmt in (M.PCAP_NANO, M.PCAPNG):
        want, off, status, counts = CC.expected(fmt, case)
        buf, boff, st, cnt = run_host(fmt, case, base=1)
        assert (boff, st, cnt) == (off, status, counts) and buf[1:1 + len(want)].tobytes() == want


def test_block_of_4gib_is_rejected():
    """GPK_CAPW_EBIG: only the sizes are computed (the data pointer is never
    followed, because no block fits out_cap = 0)."""
    L = _lib.lib()
    data = np.zeros(64, np.uint8)
    off = np.zeros(2, np.uint64)
    cap = np.array([0xFFFFFFFF - 31, 0xFFFFFFFF - 35], np.uint32)  # 28 + caplen + 4 = 2^32 and 2^32 - 4
    ci = np.zeros(2, _lib.CAPINFO_DTYPE)
    ci["length"] = 0xFFFFFFFF
    for fmt, want in ((M.PCAPNG, [M.EBIG, 0]), (M.PCAP_MICRO, [0, 0])):
        h = host_writer(fmt)
        boff, st, cnt = np.zeros(3, np.uint64), np.zeros(2, np.int32), np.zeros(4, np.uint64)
        b = _lib.Batch(data.ctypes.data, off.ctypes.data, cap.ctypes.data, 2, 64)
        _lib.check(L.gpk_capwrite_batch_host(h, ctypes.byref(b), None, 2, ci.ctypes.data, None, None, None, None, 0,
                                             boff.ctypes.data, st.ctypes.data, cnt.ctypes.data))
        L.gpk_capwriter_destroy(h)
        assert st.tolist() == want and cnt[0] == 0 and cnt[3] == 1
        assert boff[1] == (0 if want[0] else int(cap[0]) + 16)
    # the pcap formats reach 2^32 only with 16 + caplen
    h = host_writer(M.PCAP_NANO)
    cap[:] = [0xFFFFFFF0, 0xFFFFFFEF]
    _lib.check(L.gpk_capwrite_batch_host(h, ctypes.byref(b), None, 2, ci.ctypes.data, None, None, None, None, 0,
                                         boff.ctypes.data, st.ctypes.data, cnt.ctypes.data))
    L.gpk_capwriter_destroy(h)
    assert st.tolist() == [M.EBIG, 0] and int(boff[2]) == 0xFFFFFFFF


def test_builders_report_the_length_when_the_buffer_is_short():
    L = _lib.lib()
    h = host_writer(M.PCAPNG)
    f = _lib.CapwInterface()
    buf = np.full(64, 0xA5, np.uint8)
    ident = ctypes.c_int(-5)
    assert L.gpk_capwrite_add_interface(h, ctypes.byref(f), buf.ctypes.data, 8, ctypes.byref(ident)) == 32
    assert (buf == 0xA5).all() and ident.value == -5 and L.gpk_capwriter_interfaces(h) == CC.INTERFACES
    assert L.gpk_capwrite_add_interface(h, ctypes.byref(f), buf.ctypes.data, 64, ctypes.byref(ident)) == 32
    assert ident.value == CC.INTERFACES and L.gpk_capwriter_interfaces(h) == CC.INTERFACES + 1
    assert L.gpk_capwrite_file_header(h, 1, 1, buf.ctypes.data, 64) == _lib.GPK_EINVAL  # a pcapng writer
    L.gpk_capwriter_destroy(h)
    h = host_writer(M.PCAP_MICRO)
    sec = _lib.CapwSection()
    assert L.gpk_capwrite_section_header(h, ctypes.byref(sec), buf.ctypes.data, 64) == _lib.GPK_EINVAL
    assert L.gpk_capwrite_file_header(h, 1, 1, buf.ctypes.data, 23) == 24
    L.gpk_capwriter_destroy(h)
    bad = ctypes.c_void_p()
    assert L.gpk_capwriter_create(ctypes.byref(bad), 4, -1, 0) == _lib.GPK_EINVAL


# ---- layouts, the way test_abi_layout_cpu.py checks the older structs
STRUCTS = {"gpk_capw_bytes": _lib.CapwBytes, "gpk_capw_section": _lib.CapwSection,
           "gpk_capw_interface": _lib.CapwInterface, "gpk_capw_stats": _lib.CapwStats,
           "gpk_capwrite_opts": _lib.CapwriteOpts}


def test_struct_layouts_match_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_capwrite.h"', "int main(void) {",
             '  printf("{");']
    for k, (cname, mirror) in enumerate(STRUCTS.items()):
        lines.append('  printf("%s\\"%s\\": [%%zu, {", sizeof(%s));' % ("," if k else "", cname, cname))
        for j, (name, *_) in enumerate(mirror._fields_):
            lines.append('  printf("%s\\"%s\\": %%zu", offsetof(%s, %s));' % ("," if j else "", name, cname, name))
        lines.append('  printf("}]");')
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout)
    for cname, mirror in STRUCTS.items():
        assert got[cname] == [ctypes.sizeof(mirror), {n: getattr(mirror, n).offset for n, *_ in mirror._fields_}], cname
    assert _lib.CAPINFO_DTYPE.itemsize == 24
