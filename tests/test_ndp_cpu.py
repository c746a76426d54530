"""The NDP / MLD pass on the CPU (include/gpk_ndp.h): the model
against the harvested vectors and the hand-derived cases, gpk_ndp_batch_host
against the model (arrays compared whole after a 0xA5 pre-fill), the capacity
rule, argument faults, error texts, the ABI, and the Python API with the decode
oracle in place of the device."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import configs
import control_model as CM
import controlcases as CC
import dnscases as DC
import ndp_model as M
import ndpcases as C
import tunnelcases as TC
from ndputil import (CASES, CONTROLS, EXPECT, FIELD_OF, GOLDEN, GOLDEN_PACKETS, NAMES, PACKETS, ROOT, assert_same_ndp,
                     corpus, decode_and_model, err_text, model_and_host, ndp_parser)
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition

ALL_ERRORS = tuple(range(_lib.NDP_ERR_FIRST, _lib.NDP_ERR_END))


def ip6(text):
    import ipaddress
    return ipaddress.IPv6Address(text).packed


# ---- the model against what the reference's tests and source say ---------------------------------
def test_model_reproduces_hand_derived_cases():
    m, _ = decode_and_model(C.PARSER, PACKETS)
    assert set(EXPECT) <= set(NAMES)
    for i, name in enumerate(NAMES):
        e = EXPECT.get(name)
        v = int(m["verdict"][i])
        if e is None:
            assert v == _lib.NDP_NONE, name
            continue
        assert v >= 0, name
        t = m["records"][v]
        cs = [int(x) for x in m["class_start"]]
        assert (0 if v < cs[1] else 1) == e["cls"], name
        for key, want in e.items():
            if key in FIELD_OF:
                assert int(t[FIELD_OF[key]]) == want, (name, key, int(t[FIELD_OF[key]]), want)
        if "v" in e:
            assert [int(x) for x in t["v"]] == e["v"], name
        ents = m["entries"][int(t["entry0"]):int(t["entry0"]) + int(t["nentries"])]
        if "entries" in e:
            got = [(int(x["type"]), int(x["off"]), int(x["ext"])) + ((int(x["aux_off"]), int(x["aux_data_len"]), int(x["n"]))
                                                                      if len(e["entries"][0]) == 6 else ()) for x in ents]
            assert got == e["entries"], (name, got)
        if e["cls"] == 1:  # a failed message: nothing but the type, the error and where it is
            z = np.zeros(1, _lib.NDP_DTYPE)[0]
            for f in ("layer_type", "err", "err_a0", "err_a1", "status", "hdr_off"):
                z[f] = t[f]
            assert z.tobytes() == t.tobytes() and int(t["status"]) == (0 if int(t["err"]) == 154 else 1), name
    assert {int(e["err"]) for e in EXPECT.values() if e.get("err")} == set(ALL_ERRORS)  # one case per error site
    assert {e["lt"] for e in EXPECT.values() if "lt" in e and e["cls"] == 0} == set(C.LAYER_TYPES)


@pytest.mark.parametrize("v", GOLDEN, ids=[v["name"] for v in GOLDEN])
def test_model_and_hydrate_reproduce_golden(v):
    pkt = bytes.fromhex(v["hex"])
    e = v["expect"]
    p = ndp_parser()
    decoded = []
    err = p.DecodeLayers(pkt, decoded)
    assert err is None
    got = [int(t) for t in decoded]
    m, _ = decode_and_model(C.PARSER, [pkt])
    # the parser's IPv6ExtensionSkipper decodes the HopByHop header (46) without listing it
    want = [t for t in e.get("layers", []) if t != 46]
    if v["name"] == "icmp6HopByHopData":  # checkLayers ends at ICMPv6; the message layer (an MLDv2 report) follows it
        assert got[:3] == want and got[3:] == [int(m["records"][0]["layer_type"])] == [138]
        assert len(p._ndps[_lib.NDP_MLD2_REPORT].MulticastAddressRecords) == 6
        return
    if want:
        assert got == want
    lt = got[-1]
    layer = p._ndps[_lib.NDP_KIND_OF_TYPE[lt]]
    for helper, want in e.get("flags", {}).items():
        assert getattr(layer, helper)() is want, helper
    d = e.get("dissection")
    if d:
        assert p._controls[_lib.CTL_ICMP6].TypeCode.Type() == d["Type"]
        if lt in (135, 136, 137):
            assert layer.MaximumResponseDelay == d["MaximumResponseCode"] * 1000000
            assert layer.MulticastAddress == ip6(d["MulticastAddresses"][0])
            assert lt != 137 or layer.IsGeneralQuery() == (d["MulticastAddresses"][0] == "::")
        elif lt == 139:
            assert (layer.MaximumResponseCode, layer.QueriersQueryIntervalCode, layer.QueriersRobustnessVariable,
                    layer.SuppressRoutersideProcessing, layer.NumberOfSources) == (
                d["MaximumResponseCode"], d["QQIC"], d["QRV"], d["S"], d["NumberOfSources"])
            assert layer.MulticastAddress == ip6(d["MulticastAddresses"][0]) and layer.SourceAddresses == []
            assert layer.QQI() == d["QQIC"] * 1000000000 and layer.IsGeneralQuery()
        else:
            assert layer.NumberOfMulticastAddressRecords == d["NumberOfMulticastAddressRecords"]
            assert [int(r.RecordType) for r in layer.MulticastAddressRecords] == d["RecordTypes"]
            assert [r.MulticastAddress for r in layer.MulticastAddressRecords] == [ip6(a) for a in d["MulticastAddresses"]]
            assert all(r.N == 0 and r.SourceAddresses == [] and r.AuxiliaryData == b"" for r in layer.MulticastAddressRecords)
            assert layer.MulticastAddressRecords[0].RecordType.String() == "MODE_IS_EXCLUDE"


def test_golden_router_advertisement_fields():
    """The bytes of testPacketICMPv6RouterAdvertisement read by hand (the hex
    dump above it: 4000 0708 0000 0000 0000 0000, then 0101.., 0501.., 0304..):
    hop limit 64, no flags, router lifetime 1800 s, a source link-layer
    address, MTU 1500 and the prefix 2001:db8:0:1::/64."""
    v = next(v for v in GOLDEN if v["name"] == "testPacketICMPv6RouterAdvertisement")
    p = ndp_parser()
    assert p.DecodeLayers(bytes.fromhex(v["hex"]), []) is None
    ra = p._ndps[_lib.NDP_RA]
    assert (ra.HopLimit, ra.Flags, ra.RouterLifetime, ra.ReachableTime, ra.RetransTimer) == (64, 0, 1800, 0, 0)
    assert not ra.OtherConfig() and not ra.ManagedAddressConfig()
    assert [int(o.Type) for o in ra.Options][:3] == [1, 5, 3] and ra.Options[1].Data[2:] == (1500).to_bytes(4, "big")
    assert ra.Options[2].Data[0] == 64 and ra.Options[2].Data[14:] == ip6("2001:db8:0:1::")
    assert ra.Options[0].Type.String() == "SourceAddress" and L.ICMPv6Opt(77).String() == "Unknown(77)"
    assert ra.LayerContents() == bytes.fromhex(v["hex"])[58:] and ra.LayerPayload() == b""


# ---- the host entry against the model ------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_host_matches_model_on_cases_and_golden(cfg):
    m, h, _ = model_and_host(cfg, PACKETS + GOLDEN_PACKETS + list(C.layers17()), fill=0xA5)
    assert_same_ndp(m, h)
    assert int(m["counts"][1]) > 40 and int(m["counts"][2]) > 25
    assert list(m["verdict"][-2:] < 0) == [False, True] and int(m["verdict"][-1]) == _lib.NDP_UNKNOWN


def test_corpus_covers_every_outcome():
    """Asserted with the model alone."""
    pk = corpus()
    assert len(pk) == C.CORPUS_N == 2048
    m, _ = decode_and_model(C.PARSER, pk)
    n_ok, n_failed = int(m["counts"][1]), int(m["counts"][2])
    assert n_ok > len(pk) // 4 and n_failed > len(pk) // 4, (n_ok, n_failed)
    rec = m["records"][:int(m["counts"][0])]
    assert {int(x) for x in rec["err"]} - {0} == set(ALL_ERRORS)
    assert {int(x) for x in rec["layer_type"][rec["err"] == 0]} == set(C.LAYER_TYPES)
    assert int(np.sum(m["verdict"] == _lib.NDP_NONE)) > 20 and flows.NDPDecoder.needed(m["counts"]) > 500


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_host_matches_model_on_corpus(align, pad):
    m, h, _ = model_and_host(C.PARSER, corpus(), align=align, pad=pad, fill=0xA5)
    assert_same_ndp(m, h, "align %d" % align)


def test_kinds_choose_the_layers_and_the_way_in():
    """A parser without layers.ICMPv6 has no candidate behind the header; a
    kind that is not enabled is no candidate either way."""
    for kinds in (M.ALL & ~M.ICMP6, M.ICMP6 | 4, 4, M.ALL & ~4, M.ICMP6 | 32 | 256, 1023):
        m, h, _ = model_and_host(C.PARSER, PACKETS, kinds=kinds, fill=0xA5)
        assert_same_ndp(m, h, "kinds %d" % kinds)
    m, _ = decode_and_model(C.PARSER, PACKETS, kinds=M.ALL & ~M.ICMP6)
    behind = [i for i, n in enumerate(NAMES) if not n.startswith("front_") and n in EXPECT]
    front = [i for i, n in enumerate(NAMES) if n.startswith("front_")]
    assert all(int(m["verdict"][i]) == _lib.NDP_NONE for i in behind) and all(int(m["verdict"][i]) >= 0 for i in front)
    m, _ = decode_and_model(C.PARSER, PACKETS, kinds=M.ICMP6 | 4)
    got = {NAMES[i] for i in range(len(NAMES)) if int(m["verdict"][i]) >= 0}
    assert got == {n for n, e in EXPECT.items() if e.get("lt") == C.LT_NS or n in (
        "ns_one_option", "option_overruns_by_one", "icmp6_bad_checksum_still_decodes")}


def test_table_edits_reach_the_host_entry():
    """An EtherType edit that is not in the parser leaves the frame alone; one
    made on the parser alone makes it a candidate."""
    pkt = C.front(C.LT_NS, C.ns(C.opt_lladdr()))
    m0, h0, _ = model_and_host(CC.PARSER, [pkt], fill=0xA5)
    assert_same_ndp(m0, h0)
    assert list(h0["verdict"]) == [_lib.NDP_NONE]
    m1, h1, _ = model_and_host(C.PARSER, [pkt], fill=0xA5)
    assert_same_ndp(m1, h1)
    assert list(h1["verdict"]) == [0] and int(h1["records"][0]["nentries"]) == 1


# ---- capacity -----------------------------------------------------------------------------------
def test_capacity_rule():
    """Exact fit, one entry short, capacity 0, in between: a message's entries
    are written whole or not at all, nothing is written at or past the
    capacity, counts names what is needed, and the retry gets everything."""
    pk = PACKETS
    full, (data, offs, caps, ref) = decode_and_model(C.PARSER, pk)
    need = flows.NDPDecoder.needed(full["counts"])
    assert need == len(full["entries"]) and need > 20
    assert not int(full["counts"][3]) and not np.any(full["records"][:int(full["counts"][0])]["status"] & 2)
    for cap in (need, need - 1, 0, 1, need // 2, need + 3):
        m, h, _ = model_and_host(C.PARSER, pk, fill=0xA5, entry_cap=cap)
        assert_same_ndp(m, h, "cap %d" % cap)
        short = cap < need
        assert int(h["counts"][3]) == int(short) and flows.NDPDecoder.needed(h["counts"]) == need
        ok = h["records"][:int(h["counts"][1])]
        assert bool(np.any(ok["status"] & _lib.NDP_ST_DROPPED)) == short
        kept = ok[(ok["status"] & _lib.NDP_ST_DROPPED) == 0]
        assert all(int(t["entry0"]) + int(t["nentries"]) <= cap or int(t["nentries"]) == 0 for t in kept)
        assert np.array_equal(ok["entry0"], full["records"][:len(ok)]["entry0"])  # entry0 does not depend on the capacity
        for t in kept:  # what was kept is what the full run wrote
            a, b = int(t["entry0"]), int(t["entry0"]) + int(t["nentries"])
            assert h["entries"][a:b].tobytes() == full["entries"][a:b].tobytes()
        if cap > need:
            assert h["entries"][need:].tobytes() == b"\xa5" * 16 * (cap - need)
    p = configs.device_parser(C.PARSER)
    out = flows.NDPDecoder.decode_host_all(data, offs, caps, ref["records"], ref["layouts"], p, entry_cap=1)
    assert not int(out["counts"][3]) and out["entries"].tobytes() == full["entries"].tobytes()
    out = flows.NDPDecoder.decode_host_all(data, offs, caps, ref["records"], ref["layouts"], p)
    assert out["entries"].tobytes() == full["entries"].tobytes() and out["records"].tobytes() == full["records"].tobytes()


# ---- arguments, texts, ABI ----------------------------------------------------------------------
def test_host_argument_checks():
    p = configs.device_parser(C.PARSER)
    data, offs, caps = pack(PACKETS[4:6])
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    out = flows.NDPDecoder.decode_host(data[:0], offs[:0], caps[:0], ref["records"][:0], ref["layouts"][:0], p, 0)
    assert list(out["counts"]) == [0] * 8 and list(out["class_start"]) == [0] * 3
    lib = _lib.lib()
    good = flows.NDPDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], p, 8)
    ents = np.zeros(8 * 16 + 8, np.uint8)
    b = _lib.Batch(data.ctypes.data, offs.ctypes.data, caps.ctypes.data, 2, data.size)
    r = _lib.Results(ref["records"].ctypes.data, None, None, ref["layouts"].ctypes.data)

    def call(kinds=_lib.NDP_ALL, **kw):
        a = dict(verdict=good["verdict"].ctypes.data, class_start=good["class_start"].ctypes.data,
                 index=good["index"].ctypes.data, records=good["records"].ctypes.data, counts=good["counts"].ctypes.data,
                 entries=good["entries"].ctypes.data, entry_cap=8)
        a.update(kw)
        return lib.gpk_ndp_batch_host(p.h, ctypes.byref(b), ctypes.byref(r), kinds, ctypes.byref(_lib.Ndps(**a)))
    assert call() == 0
    odd = ents.ctypes.data + (4 if ents.ctypes.data % 8 == 0 else 8 - ents.ctypes.data % 8 + 4)
    for kw in (dict(verdict=None), dict(class_start=None), dict(index=None), dict(records=None), dict(counts=None),
               dict(entries=None), dict(entries=odd), dict(records=good["records"].ctypes.data + 4)):
        assert call(**kw) == _lib.GPK_EINVAL, kw
    assert call(entries=None, entry_cap=0) == 0
    for kinds in (0, _lib.NDP_ICMP6, 2048, _lib.NDP_ALL | 4096, 0x80000000):
        assert call(kinds) == _lib.GPK_EINVAL, kinds
    for kinds in (1, 512, _lib.NDP_ICMP6 | 1, _lib.NDP_MESSAGES):
        assert call(kinds) == 0, kinds
    assert lib.gpk_ndp_batch_host(None, ctypes.byref(b), ctypes.byref(r), 1, None) == _lib.GPK_EINVAL


def test_format_error_texts():
    buf = ctypes.create_string_buffer(256)
    lib = _lib.lib()
    for code in (0,) + ALL_ERRORS:
        for a0, a1 in ((0, 0), (31, 32), (56, 0), (65535, 4000000000)):
            n = lib.gpk_ndp_format_error(code, a0, a1, buf, 256)
            assert n == len(buf.value) and buf.value.decode() == M.error_text(code, a0, a1), code
    lib.gpk_ndp_format_error(147, 31, 32, buf, 256)
    assert buf.value.decode() == "ICMP layer only 31 bytes for ICMPv6 message option with length 32"
    lib.gpk_ndp_format_error(152, 9, 9, buf, 256)
    assert buf.value.decode() == ("Multicast Listener Report Message V2 layer less than 4 bytes for Multicast "
                                  "Address Record")
    lib.gpk_ndp_format_error(154, 36, 0, buf, 256)
    assert buf.value.decode() == ("Multicast Listener Report Message V2 layer less than 36 bytes for Multicast "
                                  "Address Record")
    lib.gpk_ndp_format_error(148, 0, 0, buf, 256)
    assert buf.value.decode() == "ICMP layer less than 20 bytes for Multicast Listener Query Message V1"
    texts = set()
    for code in ALL_ERRORS:
        lib.gpk_ndp_format_error(code, 1, 2, buf, 256)
        texts.add(buf.value)
    assert len(texts) == len(ALL_ERRORS) - 1 and all(t for t in texts)  # :489 and :500 share one text
    for bad in (1, 139, 155, 255):
        assert lib.gpk_ndp_format_error(bad, 0, 0, buf, 256) == _lib.GPK_EINVAL
    assert lib.gpk_ndp_format_error(146, 0, 0, buf, 8) == 7 and buf.value == b"ICMPv6 "
    assert lib.gpk_ndp_format_error(146, 0, 0, None, 8) == _lib.GPK_EINVAL


def test_abi_layout_of_ndp_structs(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler (gcc, cc or clang): the build needs a host compiler too"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_ndp.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_ndp", _lib.NDP_DTYPE), ("gpk_ndp_entry", _lib.NDP_ENTRY_DTYPE), ("gpk_ndps", _lib.Ndps)):
        if isinstance(mirror, np.dtype):
            size, fields = mirror.itemsize, {n: mirror.fields[n][1] for n in mirror.names}
        else:
            size, fields = ctypes.sizeof(mirror), {n: getattr(mirror, n).offset for n, *_ in mirror._fields_}
        want[cname] = [size] + list(fields.values())
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f in fields:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.splitlines()}
    assert got == want
    assert (_lib.NDP_DTYPE.itemsize, _lib.NDP_ENTRY_DTYPE.itemsize) == (64, 16)


def test_exports_and_constants():
    for name in ("gpk_ndp_decoder_create", "gpk_ndp_decoder_destroy", "gpk_ndp_batch", "gpk_ndp_batch_host",
                 "gpk_ndp_format_error"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "gpk_ndp.h")).read()
    for cname, val in (("GPK_NDP_RS", _lib.NDP_RS), ("GPK_NDP_MLD2_REPORT", _lib.NDP_MLD2_REPORT),
                       ("GPK_NDP_ICMP6", _lib.NDP_ICMP6), ("GPK_NDP_ALL", _lib.NDP_ALL),
                       ("GPK_NDP_ST_TRUNCATED", _lib.NDP_ST_TRUNCATED), ("GPK_NDP_ST_DROPPED", _lib.NDP_ST_DROPPED),
                       ("GPK_NDP_CLASS_FAILED", _lib.NDP_CLASS_FAILED)):
        assert re.search(r"#define %s %du?\s" % (cname, val), hdr), cname
    assert "GPK_NDP_ERR_RS_SHORT = %d," % _lib.NDP_ERR_FIRST in hdr
    assert sorted(int(c._lt) for c in L.NDP_LAYERS) == sorted(C.LAYER_TYPES) == sorted(_lib.NDP_KIND_OF_TYPE)
    assert all(M.KIND_OF_TYPE[int(c._lt)] == c.ndp_kind == _lib.NDP_KIND_OF_TYPE[int(c._lt)] for c in L.NDP_LAYERS)
    assert (int(L.ICMPv6OptRecursiveDNSServer), int(L.ICMPv6OptMTU)) == (25, 5)
    assert L.MLDv2MulticastAddressRecordTypeBlockOldSources.String() == "BLOCK_OLD_SOURCES"
    assert L.MLDv2MulticastAddressRecordType(9).String() == "UNKNOWN(9)"


# ---- the Python API, the decode oracle in place of the device -----------------------------------
def test_decode_layers_and_hydrate_every_case():
    """DecodeLayers of every case: decoded list, error text, Truncated, and the
    hydrated struct against the model's record and the packet's bytes."""
    p = ndp_parser()
    m, _ = decode_and_model(C.PARSER, PACKETS)
    composed = M.compose(C.PARSER, PACKETS)  # Truncated is the OR of the six-layer decode's and the message's
    for i, (name, pkt) in enumerate(CASES):
        decoded = []
        err = p.DecodeLayers(pkt, decoded)
        v = int(m["verdict"][i])
        if v < 0:
            assert not set(int(t) for t in decoded) & set(C.LAYER_TYPES), name
            continue
        t = m["records"][v]
        assert err_text(err) == M.error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"])), name
        assert p.Truncated == composed["truncated"][i] and (p.Truncated or not int(t["status"]) & 1), name
        lt = int(t["layer_type"])
        assert (int(decoded[-1]) == lt) == (not int(t["err"])), name
        if not name.startswith("front_"):
            assert int(decoded[-2 if not int(t["err"]) else -1]) == 57, name
        if int(t["err"]):
            continue
        d = p._ndps[_lib.NDP_KIND_OF_TYPE[lt]]
        h, ln = int(t["hdr_off"]), int(t["len"])
        msg = pkt[h:h + ln]
        assert int(d.LayerType()) == lt and d.CanDecode().Contains(lt)
        assert d.LayerContents() == (msg if lt in (125, 126, 127, 128) else b""), name
        assert d.LayerPayload() == (msg[20:] if lt == 137 else b""), name
        assert int(d.NextLayerType()) == (0 if lt in (135, 136, 137, 139) else 2), name
        ents = m["entries"][int(t["entry0"]):int(t["entry0"]) + int(t["nentries"])]
        if lt <= 128:
            assert [(int(o.Type), o.Data) for o in d.Options] == [
                (int(e["type"]), pkt[int(e["off"]):int(e["off"]) + int(e["ext"])]) for e in ents], name
            fixed = {124: 4, 125: 12, 126: 20, 127: 20, 128: 36}[lt]  # the options tile the rest of the message
            assert b"".join(bytes([int(o.Type), (len(o.Data) + 2) // 8]) + o.Data for o in d.Options) == msg[fixed:], name
        if lt in (126, 127, 128):
            assert d.TargetAddress == msg[4:20], name
        if lt in (135, 136, 137, 139):
            assert d.MulticastAddress == msg[4:20], name
        if lt == 138:
            assert len(d.MulticastAddressRecords) == d.NumberOfMulticastAddressRecords == len(ents), name
    c = dict(CASES)
    assert p.DecodeLayers(c["redirect_header_option"], []) is None
    r = p._ndps[_lib.NDP_REDIRECT]
    assert (r.TargetAddress, r.DestinationAddress) == (C.TARGET, C.DEST)
    assert r.Options == [L.ICMPv6Option(2, C.LLADDR), L.ICMPv6Option(4, bytes(6) + bytes(range(40)))]
    assert p.DecodeLayers(c["na_target_option"], []) is None
    a = p._ndps[_lib.NDP_NA]
    assert (a.Router(), a.Solicited(), a.Override(), a.Flags) == (True, True, True, 0xe0)
    assert p.DecodeLayers(c["mld2_report_2_records"], []) is None
    assert p._ndps[_lib.NDP_MLD2_REPORT].MulticastAddressRecords == [
        L.MLDv2MulticastAddressRecord(1, 1, 2, C.GROUP, [C.SRC_A, C.SRC_B], b"auxd"),
        L.MLDv2MulticastAddressRecord(4, 0, 0, C.GROUP2, [], b"")]
    assert p.DecodeLayers(c["mld2_query_two_sources"], []) is None
    q = p._ndps[_lib.NDP_MLD2_QUERY]
    assert (q.SourceAddresses, q.SuppressRoutersideProcessing, q.QueriersRobustnessVariable, q.IsSpecificQuery()) == (
        [C.SRC_A, C.SRC_B], False, 7, True)
    assert q.MaximumResponseDelay() == 10000  # mldv2.go:249-251 as written: nanoseconds below 0x8000
    q.MaximumResponseCode, q.QueriersQueryIntervalCode = 0x8123, 0x8a
    assert q.MaximumResponseDelay() == (0x123 | 0x8000) * 1000000 and q.QQI() == (0xa | 0x8000) * 1000000000
    q.MaximumResponseCode, q.QueriersQueryIntervalCode = 0x9123, 0x9a  # exp 1: the shift leaves 16 bits
    assert q.MaximumResponseDelay() == 0x123 * 1000000 and q.QQI() == 0xa * 1000000000
    assert p.DecodeLayers(c["front_mld1_query_payload"], decoded) is None and [int(t) for t in decoded] == [17, 137]
    assert p._ndps[_lib.NDP_MLD1_QUERY].LayerPayload() == b"payload!" and p._ndps[_lib.NDP_MLD1_QUERY].IsSpecificQuery()


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_composition_matches_model(cfg):
    pk = PACKETS + GOLDEN_PACKETS + corpus()[:320]
    want = M.compose(cfg, pk)
    res = G.TunnelBatchResult(ndp_parser(cfg), G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    assert len(res.levels) == 1
    w, got = want["levels"][0][0]["ndp"], res.levels[0][0].ndp
    for k in flows.NDPDecoder.KEYS:
        assert w[k].tobytes() == got[k].tobytes(), k
    t, ents = res.NDP(NAMES.index("ra_three_options"))
    assert int(t["nentries"]) == len(ents) == 3 and [int(e["type"]) for e in ents] == [1, 5, 3]
    assert res.NDP(NAMES.index("plain_udp")) is None and len(res.NDP(NAMES.index("ns_19_bytes"))[1]) == 0
    i = NAMES.index("ns_one_option")
    assert want["decoded"][i] == [17, 21, 57, 126] and want["error"][i] == ""
    with pytest.raises(ValueError, match="fields=True"):
        ndp_parser().DecodeBatch(G.PacketBatch.from_packets(PACKETS[:2]), fields=True)


def test_parser_without_icmpv6_has_no_candidate_behind_the_header():
    """The message layers without layers.ICMPv6: way 2 only."""
    pk = PACKETS
    want = M.compose(C.PARSER, pk, kinds=M.ALL & ~M.ICMP6, control_kinds=0)
    p = ndp_parser(extra=L.NDP_LAYERS)
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    i = NAMES.index("ns_one_option")
    assert want["decoded"][i] == [17, 21] and want["error"][i] == "No decoder for layer type ICMPv6"
    assert want["decoded"][NAMES.index("front_126")] == [17, 126]


def test_parser_without_the_new_layers_is_the_parents():
    """A parser that holds the control layers only gives what it gave before
    (control_model's composition): UnsupportedLayerType(...) behind ICMPv6."""
    pk = PACKETS + GOLDEN_PACKETS + corpus()[:256]
    for cfg in (C.PARSER, C.PARSER_IGNORE):
        want = CM.compose(cfg, pk)
        p = ndp_parser(cfg, extra=CONTROLS)
        assert not p._ndps
        res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
        check_composition(res, want, len(pk))
        assert all(part.ndp is None for lvl in res.levels for part in lvl) and res.NDP(0) is None
    i = NAMES.index("ns_one_option")
    want = CM.compose(C.PARSER, pk)
    assert want["decoded"][i] == [17, 21, 57] and want["error"][i] == "No decoder for layer type ICMPv6NeighborSolicitation"


def test_composition_with_control_dns_and_a_vxlan_level():
    """One parser holding the tunnel, control, message and DNS layers: the NDP
    pass runs behind the control pass on every level's part."""
    c, cc, dc = dict(CASES), dict(CC.quirk_cases()[0]), dict(DC.quirk_cases()[0])
    pk = [TC.over_udp(TC.vxlan(c["ra_three_options"]), TC.VX), c["ns_one_option"], cc["icmp4_echo"],
          TC.over_udp(TC.vxlan(cc["arp_request_42"]), TC.VX), TC.over_udp(TC.vxlan(c["option_length_0"]), TC.VX),
          dc["query_a"], cc["icmp6_echo_request"], TC.over_udp(TC.vxlan(c["mld2_report_aux_overruns"]), TC.VX),
          c["mld2_report_2_records"]]
    cfg = dict(C.PARSER, udp_port=DC.PARSER.get("udp_port"), tcp_port=DC.PARSER.get("tcp_port"))
    cfg = {k: v for k, v in cfg.items() if v is not None}
    want = M.compose(cfg, pk, control_kinds=15, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 21, 57, 125] and want["decoded"][1] == [17, 21, 57, 126]
    assert want["decoded"][2] == [17, 20, 19, 2] and want["decoded"][3] == [17, 20, 45, 116, 17, 10]
    assert want["error"][4] == "ICMPv6 message option with length 0" and want["truncated"][4]
    assert want["decoded"][4] == [17, 20, 45, 116, 17, 21, 57] and want["decoded"][6] == [17, 21, 57, 132]
    assert want["error"][7].endswith("less than 36 bytes for Multicast Address Record") and not want["truncated"][7]
    p = ndp_parser(cfg, extra=L.NDP_LAYERS + CONTROLS + (L.DNS,), tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    for i in range(len(pk)):
        if i != 5:  # the DNS query is the DNS pass's: the model of this file does not append it
            assert [int(t) for t in res.Decoded(i)] == want["decoded"][i], i
            assert err_text(res.Err(i)) == want["error"][i] and res.Truncated(i) == want["truncated"][i], i
    assert [int(t) for t in res.Decoded(5)] == [17, 20, 45, 107] and res.Err(5) is None
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._tunnels[2].VNI == 0x123456 and p._ndps[_lib.NDP_RA].RouterLifetime == 1800
    assert [int(o.Type) for o in p._ndps[_lib.NDP_RA].Options] == [1, 5, 3]
    assert p._controls[_lib.CTL_ICMP6].TypeCode.Type() == 134  # the ICMPv6 struct still comes from the control record
    assert int(p._controls[_lib.CTL_ICMP6].NextLayerType()) == 125


# ---- the example ----------------------------------------------------------------------------------
def test_neighbors_example_on_a_generated_capture(tmp_path):
    import pcapgen
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import neighbors
    c, cc = dict(CASES), dict(CC.quirk_cases()[0])
    router = bytes.fromhex("fe80000000000000021122fffe334455")
    frames = [c["ns_one_option"], c["na_target_option"], c["ra_four_options_rdnss"], cc["arp_request_42"],
              c["mld2_report_2_records"], c["mld1_report"], c["option_length_0"], c["plain_udp"],
              C.eth(C.ip6(C.icmp6(C.na(C.opt_lladdr(2, bytes.fromhex("021122334455")), target=router), 136), 58), 0x86dd)]
    path = tmp_path / "lan.pcap"
    path.write_bytes(pcapgen.pcap_file(frames))
    lines = []
    got = neighbors.run(str(path), parser=ndp_parser(), device=False, log=lines.append)
    src = "::1"  # tunnelcases.ip6's source address
    assert got["messages"] == 7 and got["failed"] == 1
    assert dict(got["neighbors"]) == {src: "00:0c:29:0e:4c:67", "fe80::20c:29ff:fe0e:4c67": "00:0c:29:0e:4c:67",
                                      "fe80::211:22ff:fe33:4455": "02:11:22:33:44:55"}
    assert list(got["arp"].items()) == [("22.23.24.25", "10:11:12:13:14:15")]
    assert dict(got["routers"]) == {src: dict(lifetime=1800, flags=0x80, prefixes=["2001:db8:0:1::/64"], mtu=1500,
                                              rdnss=["2001:db8::53"])}
    assert dict(got["listeners"]) == {src: ["ff02::1:3", "ff02::1:ffcc:e546"]}
    out = "\n".join(lines)
    assert "prefix 2001:db8:0:1::/64" in out and "mtu 1500" in out and "rdnss  2001:db8::53" in out and "(arp)" in out
