"""The UDP service pass on the CPU (include/gpk_svc.h): the model
against the harvested vectors and the hand-derived cases, gpk_svc_batch_host
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
import dnscases as DC
import ndp_model as NM
import ndpcases as NC
import svc_model as M
import svccases as C
import tunnel_model as TM
from svcutil import (CASES, CONTROLS, EXPECT, FIELD_OF, GOLDEN, GOLDEN_OPTIONS, GOLDEN_PACKETS, NAMES, PACKETS, ROOT,
                     assert_same_svc, corpus, decode_and_model, err_text, model_and_host, svc_parser)
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition

ALL_ERRORS = tuple(range(_lib.SVC_ERR_FIRST, _lib.SVC_ERR_END)) + (_lib.ERR_PANIC_SLICE_B,)


# ---- the model against what the reference's tests and source say ---------------------------------
def test_model_reproduces_hand_derived_cases():
    m, _ = decode_and_model(C.PARSER, PACKETS)
    assert set(EXPECT) <= set(NAMES)
    for i, name in enumerate(NAMES):
        e = EXPECT.get(name)
        v = int(m["verdict"][i])
        if e is None:
            assert v == _lib.SVC_NONE, name
            continue
        assert v >= 0, name
        t = m["records"][v]
        cs = [int(x) for x in m["class_start"]]
        assert (0 if v < cs[1] else 1) == e["cls"], name
        for key, want in e.items():
            if key in FIELD_OF:
                assert int(t[FIELD_OF[key]]) == want, (name, key, int(t[FIELD_OF[key]]), want)
            elif key == "b":
                assert [int(x) for x in t["b"]] == want, name
            elif key in ("v0", "v1", "v2", "v3", "v4", "v5"):
                assert int(t["v"][int(key[1])]) == want, (name, key, int(t["v"][int(key[1])]))
        ents = m["entries"][int(t["entry0"]):int(t["entry0"]) + int(t["nentries"])]
        if "entries" in e:
            assert [(int(x["code"]), int(x["length"]), int(x["off"])) for x in ents] == e["entries"], name
        if e["cls"] == 1:  # a failed message: nothing but the type, the error and where it is
            z = np.zeros(1, _lib.SVC_DTYPE)[0]
            for f in ("layer_type", "err", "err_a0", "err_a1", "status", "hdr_off"):
                z[f] = t[f]
            assert z.tobytes() == t.tobytes() and int(t["status"]) == int(int(t["err"]) in M.TRUNCATED), name
    assert {int(e["err"]) for e in EXPECT.values() if e.get("err")} == set(ALL_ERRORS)  # one case per error site
    assert {e["lt"] for e in EXPECT.values() if "lt" in e and e["cls"] == 0} == set(C.LAYER_TYPES)


def _fields_of(layer):
    out = {}
    for k, v in vars(layer).items():
        if k in ("Contents", "Payload"):
            continue
        if k == "Options":
            out[k] = [[int(getattr(o, "Type", getattr(o, "Code", 0))), o.Length, o.Data.hex()] for o in v]
        else:
            out[k] = v.hex() if isinstance(v, bytes) else int(v)
    return out


@pytest.mark.parametrize("v", GOLDEN, ids=[v["name"] for v in GOLDEN])
def test_model_and_hydrate_reproduce_golden(v):
    pkt = bytes.fromhex(v["hex"])
    e = v["expect"]
    p = svc_parser()
    decoded = []
    assert p.DecodeLayers(pkt, decoded) is None and not p.Truncated
    assert [int(t) for t in decoded] == e["layers"]
    layer = p._svcs[_lib.SVC_KIND_OF_TYPE[e["layers"][-1]]]
    assert _fields_of(layer) == e["fields"]
    h = 14 + (40 if e["layers"][1] == 21 else 20) + 8
    assert layer.LayerContents() == pkt[h:] and layer.LayerPayload() == b""
    m, _ = decode_and_model(C.PARSER, [pkt])
    assert int(m["verdict"][0]) == 0 and int(m["records"][0]["nentries"]) == len(e["fields"].get("Options", []))


@pytest.mark.parametrize("v", GOLDEN_OPTIONS, ids=[v["name"].replace(" ", "_") for v in GOLDEN_OPTIONS])
def test_golden_dhcp4_option_vectors(v):
    """TestDHCPv4DecodeOption's table: DHCPOption.decode of the buffer alone
    (the model), and the same buffer as the whole option area of a message
    (the host entry). DecodeFromBytes never hands decode an empty buffer."""
    raw, want = bytes.fromhex(v["option_hex"]), v["expect"]["error"]
    try:
        M.decode_dhcp4_option(TM.Sl(raw, 0, len(raw), len(raw)))
        got = ""
    except M.GoError as ex:
        got = M.error_text(ex.code)
    assert got == want
    if raw:
        m, h, _ = model_and_host(C.PARSER, [C.over4(C.dhcp4(raw))], fill=0xA5)
        assert_same_svc(m, h)
        t = h["records"][0]
        assert M.error_text(int(t["err"])) == want and int(t["nentries"]) == (0 if want else 1)


def test_golden_values_read_by_hand():
    """TestNTPOne's bytes by hand: d9 = LI 3, VN 3, mode 1; poll 0x0a, precision
    0xfa = -6; dispersion 0x00010290; the transmit timestamp at 40..48."""
    v = next(v for v in GOLDEN if v["name"] == "TestNTPOne")
    p = svc_parser()
    assert p.DecodeLayers(bytes.fromhex(v["hex"]), []) is None
    n = p._svcs[_lib.SVC_NTP]
    assert (n.LeapIndicator, n.Version, n.Mode, n.Stratum, n.Poll, n.Precision) == (3, 3, 1, 0, 10, -6)
    assert (n.RootDelay, n.RootDispersion, n.ReferenceID, n.TransmitTimestamp) == (0, 0x10290, 0, 0xc50204ecec42ee92)
    assert n.ExtensionBytes == b"" and int(n.NextLayerType()) == 0 and n.CanDecode().Contains(117)
    v = next(v for v in GOLDEN if v["name"] == "TestDHCPv4EncodeResponse")
    assert p.DecodeLayers(bytes.fromhex(v["hex"]), []) is None
    d = p._svcs[_lib.SVC_DHCP4]
    assert (d.Operation.String(), d.YourClientIP, d.ClientHWAddr) == ("Reply", bytes([192, 168, 0, 123]), bytes.fromhex("123456789abc"))
    assert d.Options[0] == L.DHCPOption(L.DHCPOptMessageType, 1, bytes([L.DHCPMsgTypeOffer]))
    assert d.Options[2] == L.DHCPOption(L.DHCPOptPad, 0, b"") and d.Options[2].Type.String() == "(padding)"
    assert [o.Type.String() for o in d.Options[3:]] == ["Timer1", "Timer2", "LeaseTime", "ServerID"]
    assert int(d.NextLayerType()) == 2 and L.DHCPMsgType(d.Options[0].Data[0]).String() == "Offer"


# ---- the host entry against the model ------------------------------------------------------------
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_host_matches_model_on_cases_and_golden(cfg):
    m, h, _ = model_and_host(cfg, PACKETS + GOLDEN_PACKETS + list(C.layers17()), fill=0xA5)
    assert_same_svc(m, h)
    assert int(m["counts"][1]) > 35 and int(m["counts"][2]) > 20
    assert list(m["verdict"][-2:] < 0) == [False, True] and int(m["verdict"][-1]) == _lib.SVC_UNKNOWN


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
    assert int(np.sum(m["verdict"] == _lib.SVC_NONE)) > 20 and flows.ServiceDecoder.needed(m["counts"]) > 2000


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_host_matches_model_on_corpus(align, pad):
    m, h, _ = model_and_host(C.PARSER, corpus(), align=align, pad=pad, fill=0xA5)
    assert_same_svc(m, h, "align %d" % align)


@pytest.mark.parametrize("kinds", range(1, 8))
def test_every_kinds_subset(kinds):
    """A kind that is not enabled is no candidate."""
    m, h, _ = model_and_host(C.PARSER, PACKETS, kinds=kinds, fill=0xA5)
    assert_same_svc(m, h, "kinds %d" % kinds)
    got = {NAMES[i] for i in range(len(NAMES)) if int(m["verdict"][i]) >= 0}
    assert got == {n for n, e in EXPECT.items() if "lt" in e and M.KIND_OF_TYPE[e["lt"]] & kinds} | {
        n for n in got if "lt" not in EXPECT[n]}
    assert all(M.KIND_OF_TYPE[int(t["layer_type"])] & kinds for t in m["records"][:int(m["counts"][0])])


def test_table_edits_reach_the_host_entry():
    """A registered port that is not in the parser leaves the datagram alone."""
    pkt = dict(CASES)["registered_udp_port_dhcp4"]
    m0, h0, _ = model_and_host(C.PLAIN_PARSER, [pkt], fill=0xA5)
    assert_same_svc(m0, h0)
    assert list(h0["verdict"]) == [_lib.SVC_NONE]
    m1, h1, _ = model_and_host(C.PARSER, [pkt], fill=0xA5)
    assert_same_svc(m1, h1)
    assert list(h1["verdict"]) == [0] and int(h1["records"][0]["nentries"]) == 8


# ---- capacity -----------------------------------------------------------------------------------
def test_capacity_rule():
    """Exact fit, one entry short, capacity 0, in between: a message's entries
    are written whole or not at all, nothing is written at or past the
    capacity, counts names what is needed, and the retry gets everything."""
    pk = PACKETS
    full, (data, offs, caps, ref) = decode_and_model(C.PARSER, pk)
    need = flows.ServiceDecoder.needed(full["counts"])
    assert need == len(full["entries"]) and need > 300
    assert not int(full["counts"][3]) and not np.any(full["records"][:int(full["counts"][0])]["status"] & 2)
    for cap in (need, need - 1, 0, 1, need // 2, need + 3):
        m, h, _ = model_and_host(C.PARSER, pk, fill=0xA5, entry_cap=cap)
        assert_same_svc(m, h, "cap %d" % cap)
        short = cap < need
        assert int(h["counts"][3]) == int(short) and flows.ServiceDecoder.needed(h["counts"]) == need
        ok = h["records"][:int(h["counts"][1])]
        assert bool(np.any(ok["status"] & _lib.SVC_ST_DROPPED)) == short
        kept = ok[(ok["status"] & _lib.SVC_ST_DROPPED) == 0]
        assert all(int(t["entry0"]) + int(t["nentries"]) <= cap or int(t["nentries"]) == 0 for t in kept)
        assert np.array_equal(ok["entry0"], full["records"][:len(ok)]["entry0"])  # entry0 does not depend on the capacity
        for t in kept:  # what was kept is what the full run wrote
            a, b = int(t["entry0"]), int(t["entry0"]) + int(t["nentries"])
            assert h["entries"][a:b].tobytes() == full["entries"][a:b].tobytes()
        if cap > need:
            assert h["entries"][need:].tobytes() == b"\xa5" * 8 * (cap - need)
    p = configs.device_parser(C.PARSER)
    out = flows.ServiceDecoder.decode_host_all(data, offs, caps, ref["records"], ref["layouts"], p, entry_cap=1)
    assert not int(out["counts"][3]) and out["entries"].tobytes() == full["entries"].tobytes()
    out = flows.ServiceDecoder.decode_host_all(data, offs, caps, ref["records"], ref["layouts"], p)
    assert out["entries"].tobytes() == full["entries"].tobytes() and out["records"].tobytes() == full["records"].tobytes()


# ---- arguments, texts, ABI ----------------------------------------------------------------------
def test_host_argument_checks():
    p = configs.device_parser(C.PARSER)
    i = NAMES.index("dhcp4_discover_eight_options")
    data, offs, caps = pack(PACKETS[i:i + 2])
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    out = flows.ServiceDecoder.decode_host(data[:0], offs[:0], caps[:0], ref["records"][:0], ref["layouts"][:0], p, 0)
    assert list(out["counts"]) == [0] * 8 and list(out["class_start"]) == [0] * 3
    lib = _lib.lib()
    good = flows.ServiceDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], p, 16)
    ents = np.zeros(16 * 8 + 8, np.uint8)
    b = _lib.Batch(data.ctypes.data, offs.ctypes.data, caps.ctypes.data, 2, data.size)
    r = _lib.Results(ref["records"].ctypes.data, None, None, ref["layouts"].ctypes.data)

    def call(kinds=_lib.SVC_ALL, **kw):
        a = dict(verdict=good["verdict"].ctypes.data, class_start=good["class_start"].ctypes.data,
                 index=good["index"].ctypes.data, records=good["records"].ctypes.data, counts=good["counts"].ctypes.data,
                 entries=good["entries"].ctypes.data, entry_cap=16)
        a.update(kw)
        return lib.gpk_svc_batch_host(p.h, ctypes.byref(b), ctypes.byref(r), kinds, ctypes.byref(_lib.Svcs(**a)))
    assert call() == 0
    odd = ents.ctypes.data + (4 if ents.ctypes.data % 8 == 0 else 8 - ents.ctypes.data % 8 + 4)
    for kw in (dict(verdict=None), dict(class_start=None), dict(index=None), dict(records=None), dict(counts=None),
               dict(entries=None), dict(entries=odd), dict(records=good["records"].ctypes.data + 4)):
        assert call(**kw) == _lib.GPK_EINVAL, kw
    assert call(entries=None, entry_cap=0) == 0
    for kinds in (0, 8, _lib.SVC_ALL | 8, 1 | 1024, 0x80000000):
        assert call(kinds) == _lib.GPK_EINVAL, kinds
    for kinds in range(1, 8):
        assert call(kinds) == 0, kinds
    assert lib.gpk_svc_batch_host(None, ctypes.byref(b), ctypes.byref(r), 1, None) == _lib.GPK_EINVAL


def test_format_error_texts():
    buf = ctypes.create_string_buffer(256)
    lib = _lib.lib()
    for code in (0,) + ALL_ERRORS:
        for a0, a1 in ((0, 0), (239, 12), (4, 1), (65535, 4000000000)):
            n = lib.gpk_svc_format_error(code, a0, a1, buf, 256)
            assert n == len(buf.value) and buf.value.decode() == M.error_text(code, a0, a1), code
    for code, a0, a1, text in ((160, 239, 0, "DHCPv4 length 239 too short"),
                               (161, 17, 0, "DHCPv4 hardware address length 17 exceeds 16"), (162, 0, 0, "Bad DHCP header"),
                               (163, 0, 0, "Not enough data to decode"), (164, 0, 0, "Option is malformed"),
                               (165, 3, 0, "DHCPv6 length 3 too short"),
                               (166, 33, 12, "DHCPv6 length 33 too short for message type 12"),
                               (167, 0, 0, "not enough data to decode"), (168, 2, 0, "dhcpv6 option size < length 2"),
                               (169, 0, 0, "NTP packet too short"),
                               (4, 4, 1, "panic: runtime error: slice bounds out of range [4:1]")):
        lib.gpk_svc_format_error(code, a0, a1, buf, 256)
        assert buf.value.decode() == text
    for bad in (1, 2, 3, 5, 159, 170, 255):
        assert lib.gpk_svc_format_error(bad, 0, 0, buf, 256) == _lib.GPK_EINVAL
    assert lib.gpk_svc_format_error(162, 0, 0, buf, 8) == 7 and buf.value == b"Bad DHC"
    assert lib.gpk_svc_format_error(162, 0, 0, None, 8) == _lib.GPK_EINVAL


def test_abi_layout_of_svc_structs(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler (gcc, cc or clang): the build needs a host compiler too"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_svc.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_svc", _lib.SVC_DTYPE), ("gpk_svc_entry", _lib.SVC_ENTRY_DTYPE), ("gpk_svcs", _lib.Svcs)):
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
    assert (_lib.SVC_DTYPE.itemsize, _lib.SVC_ENTRY_DTYPE.itemsize) == (64, 8)


def test_exports_and_constants():
    for name in ("gpk_svc_decoder_create", "gpk_svc_decoder_destroy", "gpk_svc_batch", "gpk_svc_batch_host",
                 "gpk_svc_format_error"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "gpk_svc.h")).read()
    for cname, val in (("GPK_SVC_DHCP4", _lib.SVC_DHCP4), ("GPK_SVC_DHCP6", _lib.SVC_DHCP6), ("GPK_SVC_NTP", _lib.SVC_NTP),
                       ("GPK_SVC_ALL", _lib.SVC_ALL), ("GPK_SVC_ST_TRUNCATED", _lib.SVC_ST_TRUNCATED),
                       ("GPK_SVC_ST_DROPPED", _lib.SVC_ST_DROPPED), ("GPK_SVC_CLASS_FAILED", _lib.SVC_CLASS_FAILED),
                       ("GPK_LT_NTP", 117), ("GPK_LT_DHCPV4", 118), ("GPK_LT_DHCPV6", 134)):
        assert re.search(r"#define %s %du?\s" % (cname, val), hdr), cname
    assert "GPK_SVC_ERR_DHCP4_SHORT = %d," % _lib.SVC_ERR_FIRST in hdr
    assert sorted(int(c._lt) for c in L.SVC_LAYERS) == sorted(C.LAYER_TYPES) == sorted(_lib.SVC_KIND_OF_TYPE)
    assert all(M.KIND_OF_TYPE[int(c._lt)] == c.svc_kind == _lib.SVC_KIND_OF_TYPE[int(c._lt)] for c in L.SVC_LAYERS)
    assert (int(L.DHCPOptHostname), int(L.DHCPOptEnd), int(L.DHCPv6OptClientID), int(L.DHCPv6OptIAPD)) == (12, 255, 1, 25)
    assert (L.DHCPOpt(53).String(), L.DHCPOpt(200).String(), L.DHCPv6Opt(3).String()) == ("MessageType", "Unknown", "IA_NA")
    assert (L.DHCPv6MsgTypeRelayForward, L.DHCPv6MsgType(13).String(), L.DHCPMsgType(9).String()) == (12, "RelayReply", "Unknown")
    assert L.DHCPMagic == 0x63825363


# ---- the Python API, the decode oracle in place of the device -----------------------------------
def test_decode_layers_and_hydrate_every_case():
    """DecodeLayers of every case: decoded list, error text, Truncated, and the
    hydrated struct against the model's record and the packet's bytes."""
    p = svc_parser()
    m, _ = decode_and_model(C.PARSER, PACKETS)
    composed = M.compose(C.PARSER, PACKETS)  # Truncated is the OR of the six-layer decode's and the message's
    for i, (name, pkt) in enumerate(CASES):
        decoded = []
        if name == "dhcp6_option_length_fffd_fits_panics":
            p.IgnorePanic = True
            with pytest.raises(G.GoPanic, match=r"slice bounds out of range \[4:1\]"):
                p.DecodeLayers(pkt, decoded)
            p.IgnorePanic = False
        err = p.DecodeLayers(pkt, decoded)
        v = int(m["verdict"][i])
        if v < 0:
            assert not set(int(t) for t in decoded) & set(C.LAYER_TYPES), name
            continue
        t = m["records"][v]
        assert err_text(err) == M.error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"])), name
        assert p.Truncated == composed["truncated"][i] and (p.Truncated or not int(t["status"]) & 1), name
        assert [int(x) for x in decoded] == composed["decoded"][i], name
        lt = int(t["layer_type"])
        assert (int(decoded[-1]) == lt) == (not int(t["err"])), name
        if int(t["err"]):
            continue
        d = p._svcs[_lib.SVC_KIND_OF_TYPE[lt]]
        h, ln = int(t["hdr_off"]), int(t["len"])
        msg = pkt[h:h + ln]
        assert int(d.LayerType()) == lt and d.CanDecode().Contains(lt) and d.LayerPayload() == b""
        assert d.LayerContents() == (b"" if lt == 118 and ln == 240 else msg), name
        assert int(d.NextLayerType()) == (0 if lt == 117 else 2), name
        if lt == 118:  # the options tile the option area up to the End
            wire = b"".join(b"\x00" if int(o.Type) == 0 else bytes([int(o.Type), o.Length]) + o.Data for o in d.Options)
            assert msg[240:240 + len(wire)] == wire and msg[240 + len(wire):240 + len(wire) + 1] in (b"", b"\xff"), name
            assert (d.ClientHWAddr, d.ServerName, d.File) == (msg[28:28 + msg[2]], msg[44:108], msg[108:236]), name
            assert d.ClientIP + d.YourClientIP + d.NextServerIP + d.RelayAgentIP == msg[12:28], name
            assert (d.Xid, d.Secs, d.Flags) == (int.from_bytes(msg[4:8], "big"), int.from_bytes(msg[8:10], "big"),
                                                int.from_bytes(msg[10:12], "big")), name
        elif lt == 134:
            relay = msg[0] in (12, 13)
            wire = b"".join(int(o.Code).to_bytes(2, "big") + o.Length.to_bytes(2, "big") + o.Data for o in d.Options)
            assert msg[34 if relay else 4:] == wire and int(d.MsgType) == msg[0], name
            assert (d.HopCount, d.LinkAddr, d.PeerAddr, d.TransactionID) == (
                (msg[1], msg[2:18], msg[18:34], b"") if relay else (0, b"", b"", msg[1:4])), name
        else:
            assert d.ExtensionBytes == msg[48:] and d.ReferenceTimestamp == int.from_bytes(msg[16:24], "big"), name
            assert d.TransmitTimestamp == int.from_bytes(msg[40:48], "big"), name
    c = dict(CASES)
    assert p.DecodeLayers(c["dhcp4_ack"], decoded) is None and [int(t) for t in decoded] == [17, 20, 45, 118]
    a = p._svcs[_lib.SVC_DHCP4]
    assert (a.ServerName.rstrip(b"\x00"), a.File.rstrip(b"\x00")) == (b"dhcp.example", b"pxelinux.0")
    assert a.Options[1] == L.DHCPOption(54, 4, bytes([10, 0, 0, 1])) and a.Options[2].Type.String() == "LeaseTime"
    assert p.DecodeLayers(c["dhcp6_relay_with_message"], decoded) is None and [int(t) for t in decoded] == [17, 21, 45, 134]
    r = p._svcs[_lib.SVC_DHCP6]
    assert (r.MsgType.String(), r.HopCount, r.LinkAddr, r.PeerAddr) == ("RelayForward", 3, C.LINK, C.PEER)
    assert r.Options == [L.DHCPv6Option(9, len(C.solicit()), C.solicit()), L.DHCPv6Option(18, 4, b"eth0")]
    assert p.DecodeLayers(c["ntp_60_bytes_extension"], decoded) is None
    n = p._svcs[_lib.SVC_NTP]
    assert (n.LeapIndicator, n.Version, n.Mode, n.Stratum, n.Precision, n.ExtensionBytes) == (3, 3, 4, 1, -23, b"extension!!!")
    assert p.DecodeLayers(c["registered_tcp_port_dhcp4"], decoded) is None and [int(t) for t in decoded] == [17, 20, 44, 118]


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_composition_matches_model(cfg):
    pk = PACKETS + GOLDEN_PACKETS + corpus()[:384]
    want = M.compose(cfg, pk)
    res = G.TunnelBatchResult(svc_parser(cfg), G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    assert len(res.levels) == 1
    w, got = want["levels"][0][0]["svc"], res.levels[0][0].svc
    for k in flows.ServiceDecoder.KEYS:
        assert w[k].tobytes() == got[k].tobytes(), k
    t, ents = res.Service(NAMES.index("dhcp4_discover_eight_options"))
    assert int(t["nentries"]) == len(ents) == 8 and [int(e["code"]) for e in ents] == [53, 61, 12, 60, 50, 55, 57, 51]
    assert res.Service(NAMES.index("plain_udp")) is None and len(res.Service(NAMES.index("dhcp4_239_bytes"))[1]) == 0
    i = NAMES.index("ntp_48_bytes")
    assert want["decoded"][i] == [17, 20, 45, 117] and want["error"][i] == ""
    i = NAMES.index("dhcp4_239_bytes")
    assert want["decoded"][i] == [17, 20, 45] and want["error"][i] == "DHCPv4 length 239 too short" and want["truncated"][i]
    with pytest.raises(ValueError, match="fields=True"):
        svc_parser().DecodeBatch(G.PacketBatch.from_packets(PACKETS[:2]), fields=True)


def test_parser_without_the_new_layers_is_the_parents():
    """A parser without DHCPv4, DHCPv6 and NTP gives what it gave before: the
    six-layer decode's composition (tunnel_model's without tunnels), the
    control layers' (control_model's) and the NDP layers' (ndp_model's), with
    UnsupportedLayerType(...) in front of the three."""
    pk = PACKETS + GOLDEN_PACKETS + corpus()[:256]
    for cfg in (C.PARSER, C.PARSER_IGNORE):
        for extra, want in ((CONTROLS, CM.compose(cfg, pk)), (L.NDP_LAYERS + CONTROLS, NM.compose(cfg, pk))):
            p = svc_parser(cfg, extra=extra)
            assert not p._svcs
            res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
            check_composition(res, want, len(pk))
            assert all(part.svc is None for lvl in res.levels for part in lvl) and res.Service(0) is None
    assert not svc_parser(C.PARSER, extra=())._post_passes()  # and a parser with none of them takes the plain path
    p = svc_parser(C.PARSER, extra=CONTROLS)
    decoded = []
    assert err_text(p.DecodeLayers(dict(CASES)["ntp_48_bytes"], decoded)) == "No decoder for layer type NTP"
    assert [int(t) for t in decoded] == [17, 20, 45]
    assert err_text(p.DecodeLayers(dict(CASES)["dhcp4_ack"], decoded)) == "No decoder for layer type DHCPv4"
    assert err_text(p.DecodeLayers(dict(CASES)["dhcp6_solicit_five_options"], decoded)) == "No decoder for layer type DHCPv6"


def test_composition_with_dns_ndp_and_a_vxlan_level():
    """One parser holding the tunnel, control, NDP, DNS and service layers: the
    service pass runs on every level's part, and the passes' candidates are
    disjoint."""
    c, nc, dc = dict(CASES), dict(NC.quirk_cases()[0]), dict(DC.quirk_cases()[0])
    pk = [C.over_udp(C.vxlan(c["dhcp4_ack"]), C.VX), c["dhcp4_discover_eight_options"], nc["ra_three_options"],
          C.over_udp(C.vxlan(c["dhcp6_7_bytes"]), C.VX), c["ntp_48_bytes"], dc["query_a"],
          C.over_udp(C.vxlan(c["ntp_47_bytes"]), C.VX), c["behind_vxlan_dhcp4"], nc["ns_one_option"],
          c["dhcp6_solicit_five_options"], C.over_udp(C.vxlan(nc["ns_one_option"]), C.VX)]
    cfg = dict(C.PARSER, tcp_port=dict(list(C.TCP_EDIT.items()) + list(DC.PARSER["tcp_port"].items())))
    want = M.compose(cfg, pk, base=NM.compose(cfg, pk, control_kinds=15, tunnel_kinds=7))
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 20, 45, 118] and want["decoded"][1] == [17, 20, 45, 118]
    assert want["decoded"][2] == [17, 21, 57, 125] and want["decoded"][4] == [17, 20, 45, 117]
    assert want["error"][3] == "not enough data to decode" and not want["truncated"][3]
    assert want["decoded"][3] == [17, 20, 45, 116, 17, 21, 45]
    assert want["error"][6] == "NTP packet too short" and want["truncated"][6]
    assert want["decoded"][10] == [17, 20, 45, 116, 17, 21, 57, 126]
    p = svc_parser(cfg, extra=L.SVC_LAYERS + L.NDP_LAYERS + CONTROLS + (L.DNS,), tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    for i in range(len(pk)):
        if i != 5:  # the DNS query is the DNS pass's: the models used here do not append it
            assert [int(t) for t in res.Decoded(i)] == want["decoded"][i], i
            assert err_text(res.Err(i)) == want["error"][i] and res.Truncated(i) == want["truncated"][i], i
    assert [int(t) for t in res.Decoded(5)] == [17, 20, 45, 107] and res.Err(5) is None
    for lvl in res.levels:  # disjoint: no packet is a candidate of two passes
        for part in lvl:
            both = (part.svc["verdict"] >= 0) & ((part.ndp["verdict"] >= 0) | (part.dns["verdict"] >= 0))
            assert not both.any()
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._tunnels[2].VNI == 0x123456 and p._svcs[_lib.SVC_DHCP4].YourClientIP == bytes([10, 0, 0, 99])
    assert [int(o.Type) for o in p._svcs[_lib.SVC_DHCP4].Options] == [53, 54, 51, 1, 3]
    assert res.Service(0)[0]["hdr_off"] == C.HDR and res.Service(2) is None and res.NDP(2) is not None


# ---- the example ----------------------------------------------------------------------------------
def test_leases_example_on_a_generated_capture(tmp_path):
    import pcapgen
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import leases
    c = dict(CASES)
    frames = [c["dhcp4_discover_eight_options"], c["dhcp4_ack"], c["dhcp6_solicit_five_options"], c["ntp_48_bytes"],
              c["ntp_server_reply"], c["dhcp4_bad_magic"], c["plain_udp"], c["dhcp6_reply_from_server"]]
    path = tmp_path / "lan.pcap"
    path.write_bytes(pcapgen.pcap_file(frames))
    lines = []
    got = leases.run(str(path), parser=svc_parser(), device=False, log=lines.append)
    assert got["messages"] == 7 and got["failed"] == 1
    mac = "00:0c:29:a1:b2:c3"
    assert list(got["clients"]) == [mac]
    assert got["clients"][mac] == dict(hostname="host-1", requested="10.0.0.99", assigned="10.0.0.99",
                                       types=["Discover", "Ack"], server="10.0.0.1", lease=86400, vendor="MSFT 5.0")
    assert got["duids"] == {"1a2b3c": C.DUID.hex()}
    assert got["ntp"] == {"10.0.0.1": dict(stratum=1, version=4)}  # tunnelcases.ip4's source address, the reply's
    out = "\n".join(lines)
    assert "host-1" in out and "lease 86400" in out and "stratum 1" in out and C.DUID.hex() in out
