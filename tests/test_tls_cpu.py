"""TLS decode without a GPU: the model (tls_model.py) against the pins harvested
from the reference's tests and the hand-derived cases, then gpk_tls_batch_host
(the C++ the kernels run, on the calling thread) against the model on every
case and on the seeded corpus, byte for byte, the capacity rules, argument
faults, error texts, the ABI layout, and the composition through the Python
parser with the decode oracle in place of the device: DecodeLayers, Hydrate, a
VXLAN level, the control layers and DNS beside it, SNIs() and
examples/snilist.py."""
import collections
import ctypes
import importlib.util
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import configs
import controlcases as CC
import dnscases as DC
import tls_model as M
import tlscases as C
import tunnelcases as TC
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tlsutil import (GOLDEN, assert_same_tls, decode_and_model, err_text, golden_packet, model_and_host, tls_parser)
from tunnelutil import check_composition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, EXPECT = C.quirk_cases()
PACKETS = [p for _, p in CASES]
NAMES = [n for n, _ in CASES]


def hydrated(pkt, parser=None):
    """(error, decoded types, the TLS struct) of DecodeLayers on one packet."""
    p = parser or tls_parser()
    decoded = []
    err = p.DecodeLayers(pkt, decoded)
    return err, [int(t) for t in decoded], p._tls


def entries(m, i):
    """(message record, its record entries, its hello entries, its server names or None) of packet i."""
    t = m["records"][int(m["verdict"][i])]
    recs = m["recs"][int(t["rec0"]):int(t["rec0"]) + int(t["nrec"])]
    hel = m["hellos"][int(t["hello0"]):int(t["hello0"]) + int(t["nhello"])]
    names = [bytes(m["snis"][int(h["sni_pos"]):int(h["sni_pos"]) + int(h["sni_len"])]) if int(h["has_sni"]) else None
             for h in hel]
    return t, recs, hel, names


def from_golden(x):
    """A harvested value: {"hex": ...} is bytes, the rest stays."""
    return bytes.fromhex(x["hex"]) if isinstance(x, dict) and set(x) == {"hex"} else x


def same_bytes(got, want):
    """reflect.DeepEqual of two []byte: nil equals nil only, empty equals empty."""
    want = from_golden(want)
    return got is None if want is None else got is not None and bytes(got) == want


def assert_struct(got, want, path="TLS"):
    """A hydrated dataclass (or the TLS layer) against a harvested struct, field for field;
    a field the literal leaves out is the type's zero value."""
    for key, w in want.items():
        g = getattr(got, key) if key != "BaseLayer" else got
        if key == "BaseLayer":
            assert same_bytes(g.Contents, w["Contents"]), path + ".Contents"
            assert w["Payload"] is None and g.LayerPayload() == b"", path + ".Payload"
        elif isinstance(w, list):
            assert len(g) == len(w), (path, key, len(g), len(w))
            for k, (a, b) in enumerate(zip(g, w)):
                assert_struct(a, b, "%s.%s[%d]" % (path, key, k))
        elif w is None and isinstance(g, list):
            assert g == [], (path, key)  # a nil slice of records
        elif isinstance(w, dict) and set(w) != {"hex"}:
            assert_struct(g, w, path + "." + key)
        elif isinstance(w, dict) or w is None:
            assert same_bytes(g, w), (path, key, g, w)
        else:
            assert int(g) == w, (path, key, g, w)


def zero_fields(rec):
    """The fields of a hydrated record that no literal key names must be zero values: checked for ClientHello."""
    return all(v in (0, None, b"") for v in vars(rec).values())


# ---- the model against the reference's own pins -------------------------------------
@pytest.mark.parametrize("v", GOLDEN, ids=[v["name"] for v in GOLDEN])
def test_model_and_hydrate_reproduce_golden(v):
    """Each harvested vector through the model and through DecodeLayers +
    Hydrate (the host entry): an error where the Go test wants one, else the
    layer list and every field of the struct literal the test compares with."""
    pkt, at = golden_packet(v)
    e = v["expect"]
    m, _ = decode_and_model(C.PARSER, [pkt])
    assert int(m["counts"][0]) == 1 and int(m["records"][0]["hdr_off"]) == at
    err, decoded, d = hydrated(pkt)
    t = m["records"][0]
    assert err_text(err) == M.error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"]))
    if e is None:  # no Go test decodes it: the outcome by hand from the rules
        want = {"testServerHello": M.E_HS_TYPE, "testNewSessionTicket": 0}[v["name"]]
        assert int(t["err"]) == want
        return
    if e["error"]:
        assert int(t["err"]) and err is not None and decoded[-1] != 140
        return
    assert not int(t["err"]) and err is None and decoded == [17, 20, 44, 140]
    if e["layers"] and len(e["layers"]) > 1:
        assert e["layers"] == ["Ethernet", "IPv4", "TCP", "TLS"]
    assert_struct(d, e["decoded"])
    for r in d.Handshake:  # the literals leave ClientHello out where the Go struct holds its zero value
        if not any("ClientHello" in w for w in e["decoded"]["Handshake"] or []):
            assert zero_fields(r.ClientHello)


def test_golden_client_hello_by_value():
    v = next(x for x in GOLDEN if x["name"] == "testClientHello")
    m, _ = decode_and_model(C.PARSER, [bytes.fromhex(v["hex"])])
    t, recs, hel, names = entries(m, 0)
    assert names == [b"www.google.com"] and int(t["nhandshake"]) == int(t["nrec"]) == int(t["nhello"]) == 1
    assert (int(hel[0]["length"]), int(hel[0]["cipher_suits_length"]), int(hel[0]["extensions_length"])) == (0xcd, 0x5a, 0x60)
    assert int(recs[0]["hs"]) == _lib.TLS_HS_CLIENT_HELLO and int(recs[0]["hello"]) == 0


def test_model_reproduces_hand_derived_cases():
    m, _ = decode_and_model(C.PARSER, PACKETS)
    for i, name in enumerate(NAMES):
        exp, v = EXPECT[name], int(m["verdict"][i])
        if not exp:
            assert v == _lib.TLS_NONE, name
            continue
        assert v >= 0, name
        t, recs, hel, names = entries(m, i)
        assert (int(t["err"]), int(t["err_a0"]), int(t["err_a1"])) == (exp["err"], exp.get("a0", 0), exp.get("a1", 0)), name
        assert int(t["status"]) == exp.get("status", 0), name
        assert (v >= int(m["class_start"][1])) == bool(exp["err"]), name
        if exp["err"]:
            assert t.tobytes()[16:] == bytes(64) and int(t["hdr_off"]) > 0, name  # everything else is 0
            continue
        for key, field in (("kinds", "content_type"), ("hs", "hs"), ("v0", "v0"), ("v1", "v1")):
            if key in exp:
                assert [int(x) for x in recs[field]] == exp[key], (name, key)
        if "sni" in exp:
            assert names == exp["sni"], (name, names)
        assert int(t["nrec"]) == len(recs) == sum(int(t[k]) for k in ("nccs", "nalert", "nhandshake", "nappdata"))
    assert {EXPECT[n]["err"] for n in NAMES if EXPECT[n]} >= set(M.ALL_ERRORS)  # one case per error code at least
    assert int(entries(m, NAMES.index("appdata_300_empty"))[0]["nappdata"]) == 300


# ---- the host entry against the model --------------------------------------------------
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_host_matches_model_on_cases_and_golden(cfg):
    pk = PACKETS + [golden_packet(v)[0] for v in GOLDEN] + list(C.layers17())
    m, h, _ = model_and_host(cfg, pk, fill=0xA5)
    assert_same_tls(m, h, "cases")
    assert int(m["counts"][1]) > 40 and int(m["counts"][2]) > 40 and not int(m["counts"][3])
    assert list(m["verdict"][-2:]) == [int(m["class_start"][1]) - 1, _lib.TLS_UNKNOWN]  # 16 layers decode, 17 do not


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


def test_fuzz_corpus_covers_every_outcome(fuzz):
    """With the model alone: every error code occurs (none was shown
    unreachable among those that have a code), at least a third of the
    candidates decode, at least 50 ClientHellos carry a server name."""
    m, _ = decode_and_model(C.PARSER, fuzz)
    n = int(m["counts"][0])
    errs = collections.Counter(int(e) for e in m["records"][:n]["err"])
    for code in M.ALL_ERRORS:
        assert errs[code] > 0, (code, errs)
    assert int(m["counts"][1]) * 3 >= n, m["counts"]
    assert int(np.count_nonzero(m["hellos"]["has_sni"])) >= 50
    assert np.count_nonzero(m["verdict"] == _lib.TLS_NONE) > 0 and len(fuzz) >= 2000


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_host_matches_model_on_fuzz(fuzz, align, pad):
    m, h, _ = model_and_host(C.PARSER, fuzz, align=align, pad=pad, fill=0xA5)
    assert_same_tls(m, h, "fuzz")


def test_table_edits_reach_the_host_entry():
    """TCP port 8443 is a TLS port only in a parser with the edit."""
    pk = [dict(CASES)["registered_port_8443"], dict(CASES)["appdata_1"]]
    m, h, _ = model_and_host(C.PARSER, pk)
    assert_same_tls(m, h)
    assert list(h["verdict"]) == [0, 1]
    m0, h0, _ = model_and_host(dict(C.PARSER, tcp_port=None), pk)
    assert_same_tls(m0, h0)
    assert list(h0["verdict"]) == [_lib.TLS_NONE, 0]


# ---- capacities -------------------------------------------------------------------------------
def test_capacity_rules():
    """Exact fit, one short and zero in each arena separately: a message is
    written whole or not at all, nothing is written at or past a capacity,
    counts names what is needed, and the retry helper gets everything."""
    c = dict(CASES)
    pk = [c[k] for k in ("appdata_2", "hello_with_sni", "four_kinds", "two_hellos", "length_one_short", "sni_absent",
                         "hello_spills_into_next_record", "ccs_message_1", "sni_twice_last_wins", "plain_tcp_port_80")]
    full, (data, offs, caps, ref) = decode_and_model(C.PARSER, pk)
    need = flows.TLSDecoder.needed(full["counts"])
    assert need == (len(full["recs"]), len(full["hellos"]), len(full["snis"])) and need[0] > 12 and need[1] > 5
    assert need[2] > 40 and not int(full["counts"][3])
    assert not np.any(full["records"][:int(full["counts"][0])]["status"] & 2)
    trials = [need, (0, 0, 0), tuple(x // 2 for x in need), tuple(x + 3 for x in need)]
    for k in range(3):
        trials += [tuple(x - (j == k) for j, x in enumerate(need)), tuple(0 if j == k else x for j, x in enumerate(need))]
    for caps3 in trials:
        m, h, _ = model_and_host(C.PARSER, pk, fill=0xA5, caps3=caps3)
        assert_same_tls(m, h, "caps %r" % (caps3,))
        short = any(a < b for a, b in zip(caps3, need))
        assert int(h["counts"][3]) == int(short) and flows.TLSDecoder.needed(h["counts"]) == need
        ok = h["records"][:int(h["counts"][1])]
        assert bool(np.any(ok["status"] & _lib.TLS_ST_DROPPED)) == short
        kept = ok[(ok["status"] & _lib.TLS_ST_DROPPED) == 0]
        assert all(int(t["rec0"]) + int(t["nrec"]) <= caps3[0] and int(t["hello0"]) + int(t["nhello"]) <= caps3[1] and
                   int(t["sni0"]) + int(t["sni_bytes"]) <= caps3[2] for t in kept)
        for t in kept:  # what was kept is what the full run wrote
            a, b = int(t["rec0"]), int(t["rec0"]) + int(t["nrec"])
            assert h["recs"][a:b].tobytes() == full["recs"][a:b].tobytes()
            a, b = int(t["hello0"]), int(t["hello0"]) + int(t["nhello"])
            assert h["hellos"][a:b].tobytes() == full["hellos"][a:b].tobytes()
    p = configs.device_parser(C.PARSER)
    out = flows.TLSDecoder.decode_host_all(data, offs, caps, ref["records"], ref["layouts"], p, 1, 1, 1)
    assert not int(out["counts"][3])
    for k in ("recs", "hellos", "snis"):
        assert out[k].tobytes() == full[k].tobytes(), k


def test_host_argument_checks():
    p = configs.device_parser(C.PARSER)
    data, offs, caps = pack([dict(CASES)["hello_with_sni"], dict(CASES)["appdata_2"]])
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    out = flows.TLSDecoder.decode_host(data[:0], offs[:0], caps[:0], ref["records"][:0], ref["layouts"][:0], p, 0, 0, 0)
    assert list(out["counts"]) == [0] * 12 and list(out["class_start"]) == [0] * 3
    lib = _lib.lib()
    good = flows.TLSDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], p, 8, 4, 64)
    assert flows.TLSDecoder.needed(good["counts"]) == (3, 1, 11) and not int(good["counts"][3])
    spare = np.zeros(8 * 64 + 8, np.uint8)
    odd = spare.ctypes.data + (4 if spare.ctypes.data % 8 == 0 else 8 - spare.ctypes.data % 8 + 4)
    b = _lib.Batch(data.ctypes.data, offs.ctypes.data, caps.ctypes.data, 2, data.size)
    r = _lib.Results(ref["records"].ctypes.data, None, None, ref["layouts"].ctypes.data)

    def call(**kw):
        a = dict(verdict=good["verdict"].ctypes.data, class_start=good["class_start"].ctypes.data,
                 index=good["index"].ctypes.data, records=good["records"].ctypes.data, counts=good["counts"].ctypes.data,
                 recs=good["recs"].ctypes.data, hellos=good["hellos"].ctypes.data, snis=good["snis"].ctypes.data,
                 rec_cap=8, hello_cap=4, sni_cap=64)
        a.update(kw)
        return lib.gpk_tls_batch_host(p.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(_lib.Tlss(**a)))
    assert call() == 0
    for kw in (dict(verdict=None), dict(class_start=None), dict(index=None), dict(records=None), dict(counts=None),
               dict(recs=None), dict(hellos=None), dict(snis=None), dict(recs=odd), dict(hellos=odd),
               dict(records=good["records"].ctypes.data + 4)):
        assert call(**kw) == _lib.GPK_EINVAL, kw
    assert call(recs=None, rec_cap=0) == 0 and call(hellos=None, hello_cap=0) == 0 and call(snis=None, sni_cap=0) == 0
    assert lib.gpk_tls_batch_host(None, ctypes.byref(b), ctypes.byref(r), None) == _lib.GPK_EINVAL


def test_format_error_texts():
    buf = ctypes.create_string_buffer(256)
    lib = _lib.lib()
    for code in (0,) + M.ALL_ERRORS:
        for a0, a1 in ((0, 0), (9, 1), (9, 8), (65535, 4000000000)):
            n = lib.gpk_tls_format_error(code, a0, a1, buf, 256)
            assert n == len(buf.value) and buf.value.decode() == M.error_text(code, a0, a1), code
    lib.gpk_tls_format_error(4, 9, 1, buf, 256)
    assert buf.value.decode() == "panic: runtime error: slice bounds out of range [9:1]"
    texts = set()
    for code in range(_lib.TLS_ERR_FIRST, _lib.TLS_ERR_END):
        lib.gpk_tls_format_error(code, 0, 0, buf, 256)
        texts.add(buf.value.decode())
    # the texts of errors.New in the five files, the one that cannot occur left out
    ref_texts = {"TLS record too short", "Unknown TLS record type", "TLS packet length mismatch",
                 "TLS Change Cipher Spec record incorrect length", "TLS Alert packet too short",
                 "TLS handshake record too short", "Unknown TLS handshake type", "TLS ClientHello too short",
                 "TLS ClientHello truncated in session ID", "TLS ClientHello truncated in cipher suites",
                 "TLS ClientHello truncated in compression methods", "TLS ClientHello truncated in extensions"}
    assert texts == ref_texts
    for bad in (1, 2, 3, 5, 120, 133, 255):
        assert lib.gpk_tls_format_error(bad, 0, 0, buf, 256) == _lib.GPK_EINVAL
    assert lib.gpk_tls_format_error(121, 0, 0, buf, 8) == 7 and buf.value == b"TLS rec"
    assert lib.gpk_tls_format_error(121, 0, 0, None, 8) == _lib.GPK_EINVAL


def test_abi_layout_of_tls_structs(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler (gcc, cc or clang): the build needs a host compiler too"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_tls.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_tls", _lib.TLS_DTYPE), ("gpk_tls_rec", _lib.TLS_REC_DTYPE),
                          ("gpk_tls_hello", _lib.TLS_HELLO_DTYPE), ("gpk_tlss", _lib.Tlss)):
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
    assert (_lib.TLS_DTYPE.itemsize, _lib.TLS_REC_DTYPE.itemsize, _lib.TLS_HELLO_DTYPE.itemsize) == (80, 16, 64)


def test_exports_and_constants():
    for name in ("gpk_tls_decoder_create", "gpk_tls_decoder_destroy", "gpk_tls_batch", "gpk_tls_batch_host",
                 "gpk_tls_format_error"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "gpk_tls.h")).read()
    for cname, val in (("GPK_LT_TLS", _lib.LT_TLS), ("GPK_TLS_ST_TRUNCATED", _lib.TLS_ST_TRUNCATED),
                       ("GPK_TLS_ST_DROPPED", _lib.TLS_ST_DROPPED), ("GPK_TLS_CLASS_FAILED", _lib.TLS_CLASS_FAILED),
                       ("GPK_TLS_HS_CLIENT_KEY", _lib.TLS_HS_CLIENT_KEY), ("GPK_TLS_NO_HELLO", "0xFFFFFFFF")):
        assert re.search(r"#define %s %su?\s" % (cname, val), hdr), cname
    assert "GPK_TLS_ERR_RECORD_SHORT = %d," % _lib.TLS_ERR_FIRST in hdr and int(L.LayerTypeTLS) == 140
    assert _lib.TLS_ERR_FIRST == _lib.DNS_ERR_END and _lib.TLS_ERR_END - _lib.TLS_ERR_FIRST == 12
    dns = open(os.path.join(ROOT, "include", "gpk_dns.h")).read()
    assert re.search(r"GPK_ERR_PANIC_SLICE_B = %d," % _lib.ERR_PANIC_SLICE_B, open(os.path.join(ROOT, "include", "gpk.h")).read())
    assert "GPK_DNS_ERR_END" in dns


def test_type_strings():
    """The reference's String() values (tls.go, tls_alert.go, tls_cipherspec.go)."""
    assert [L.TLSType(x).String() for x in (20, 21, 22, 23, 19, 255)] == [
        "Change Cipher Spec", "Alert", "Handshake", "Application Data", "Unknown", "Unknown"]
    assert [L.TLSVersion(x).String() for x in (0x0200, 0x0300, 0x0301, 0x0302, 0x0303, 0x0304, 0x0305)] == [
        "SSL 2.0", "SSL 3.0", "TLS 1.0", "TLS 1.1", "TLS 1.2", "TLS 1.3", "Unknown"]
    assert [L.TLSAlertLevel(x).String() for x in (1, 2, 3, 255)] == ["Warning", "Fatal", "Unknown(3)", "Unknown(255)"]
    assert [L.TLSAlertDescr(x).String() for x in (0, 40, 110, 111, 255)] == [
        "close_notify", "handshake_failure", "unsupported_extension", "Unknown", "Unknown"]
    assert [L.TLSchangeCipherSpec(x).String() for x in (1, 255, 0)] == ["Change Cipher Spec Message", "Unknown", "Unknown"]
    assert (int(L.TLSApplicationData), int(L.TLSAlertUnknownLevel), int(L.TLSChangecipherspecUnknown),
            L.TLSHandshakeClientKeyExchange) == (23, 255, 255, 16)


# ---- the Python API, the decode oracle in place of the device -----------------------------------
def test_decode_layers_and_hydrate_every_case():
    """DecodeLayers of every case: decoded list, error text, Truncated, and
    the hydrated struct against the model's entries."""
    p = tls_parser()
    m, _ = decode_and_model(C.PARSER, PACKETS)
    for i, (name, pkt) in enumerate(CASES):
        decoded = []
        err = p.DecodeLayers(pkt, decoded)
        v = int(m["verdict"][i])
        if v < 0:
            assert 140 not in [int(t) for t in decoded], name
            continue
        t, recs, hel, names = entries(m, i)
        assert err_text(err) == M.error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"])), name
        assert p.Truncated == bool(int(t["status"]) & 1), name
        assert (int(decoded[-1]) == 140) == (not int(t["err"])), name
        if int(t["err"]):
            continue
        d = p._tls
        last = int(recs[-1]["body_off"]) - 5
        assert d.LayerContents() == pkt[last:int(t["hdr_off"]) + int(t["len"])] and d.LayerPayload() == b"", name
        assert (len(d.ChangeCipherSpec), len(d.Alert), len(d.Handshake), len(d.AppData)) == (
            int(t["nccs"]), int(t["nalert"]), int(t["nhandshake"]), int(t["nappdata"])), name
        assert [r.ClientHello.SNI for r in d.Handshake if r.ClientHello.HandshakeType == 1] == names, name
        for lst, ct in ((d.ChangeCipherSpec, 20), (d.Alert, 21), (d.Handshake, 22), (d.AppData, 23)):
            want = recs[recs["content_type"] == ct]
            assert [(int(r.TLSRecordHeader.ContentType), int(r.TLSRecordHeader.Version), r.TLSRecordHeader.Length)
                    for r in lst] == [(ct, int(w["version"]), int(w["length"])) for w in want], name
        assert [r.Payload for r in d.AppData] == [pkt[int(w["body_off"]):int(w["body_off"]) + int(w["length"])]
                                                  for w in recs[recs["content_type"] == 23]], name


def test_hydrated_fields_by_hand():
    c = dict(CASES)
    _, decoded, d = hydrated(c["four_kinds"])
    assert decoded == [17, 20, 44, 140]
    assert d.ChangeCipherSpec == [L.TLSChangeCipherSpecRecord(L.TLSRecordHeader(20, 0x0303, 1), 1)]
    assert d.Alert == [L.TLSAlertRecord(L.TLSRecordHeader(21, 0x0303, 2), 2, 40, None)]
    assert d.Alert[0].Level.String() == "Fatal" and d.Alert[0].Description.String() == "handshake_failure"
    assert d.AppData == [L.TLSAppDataRecord(L.TLSRecordHeader(23, 0x0303, 4), b"data")]
    assert [r.TLSRecordHeader.Length for r in d.Handshake] == [20, 40] and all(zero_fields(r.ClientHello) for r in d.Handshake)
    a = hydrated(c["alert_length_3_is_encrypted"])[2].Alert[0]
    assert (int(a.Level), int(a.Description), a.EncryptedMsg) == (255, 255, b"\x02\x28\x00")
    assert hydrated(c["ccs_message_2_is_255"])[2].ChangeCipherSpec[0].Message.String() == "Unknown"
    h = hydrated(c["hello_with_sni"])[2].Handshake[0]
    assert h.TLSRecordHeader.Version.String() == "TLS 1.0" and h.TLSRecordHeader.ContentType.String() == "Handshake"
    ch = h.ClientHello
    assert (ch.HandshakeType, ch.ProtocolVersion, ch.Random, ch.SessionIDLength, ch.SessionID, ch.CipherSuitsLength,
            ch.CipherSuits, ch.CompressionMethodsLength, ch.CompressionMethods, ch.SNI) == (
        1, 0x0303, bytes(range(32)), 0, b"", 4, b"\x13\x01\x13\x02", 1, b"\x00", b"example.com")
    assert ch.Extensions == C.sni_ext() + C.ALPN and ch.ExtensionsLength == len(ch.Extensions) and ch.Length == 34 + 11 + len(ch.Extensions)
    ch = hydrated(c["hello_spills_into_next_record"])[2].Handshake[0].ClientHello
    assert (ch.Length, ch.ProtocolVersion, ch.Random[:3], ch.SNI) == (0, 0x1703, b"\x03" + struct.pack(">H", 29 + len(
        C.hello_tail(C.sni_ext(b"spill.test")))), b"spill.test")
    assert hydrated(c["sni_empty_hostname"])[2].Handshake[0].ClientHello.SNI == b""
    assert hydrated(c["sni_absent"])[2].Handshake[0].ClientHello.SNI is None
    d = hydrated(c["appdata_1"])[2]
    assert d.CanDecode().Contains(L.LayerTypeTLS) and int(d.NextLayerType()) == 0 and int(d.LayerType()) == 140
    with pytest.raises(NotImplementedError):
        d.SerializeTo(None, None)


def test_panic_is_an_error_or_a_panic():
    """DecodeLayers turns the slice panic into an error; with IgnorePanic it is raised."""
    pkt = dict(CASES)["sni_hostname_length_fff8_panics"]
    err, decoded, _ = hydrated(pkt)
    assert err_text(err) == "panic: runtime error: slice bounds out of range [9:1]" and decoded == [17, 20, 44]
    p = tls_parser()
    p.IgnorePanic = True
    with pytest.raises(G.GoPanic, match=r"slice bounds out of range \[9:1\]"):
        p.DecodeLayers(pkt, [])


def test_with_and_without_the_layer():
    """[Ethernet IPv4 TCP TLS] when the parser holds layers.TLS, and [Ethernet
    IPv4 TCP] + UnsupportedLayerType(TLS) when it does not; 8443 only with
    the table edit."""
    pkt = dict(CASES)["appdata_2"]
    err, decoded, d = hydrated(pkt)
    assert err is None and decoded == [17, 20, 44, 140] and len(d.AppData) == 2
    p = tls_parser(extra=())
    assert p._tls is None and p._dns is None and not p._controls and not p._tunnels and not p._post_passes()
    assert sorted(p._decoders) == list(range(1, 9))
    q = tls_parser(extra=(L.DNS,))  # a post-pass parser without layers.TLS
    res = G.TunnelBatchResult(q, G.PacketBatch.from_packets([pkt]), device=False)
    assert err_text(res.Err(0)) == "No decoder for layer type TLS" and res.TLS(0) is None and res.SNIs() == []
    assert [int(t) for t in res.Decoded(0)] == [17, 20, 44]
    err, decoded, _ = hydrated(dict(CASES)["registered_port_8443"], tls_parser(dict(C.PARSER, tcp_port=None)))
    assert decoded == [17, 20, 44, 2] and err is None  # gopacket.Payload
    with pytest.raises(ValueError, match="fields=True"):
        tls_parser().DecodeBatch(G.PacketBatch.from_packets(PACKETS[:2]), fields=True)


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_composition_matches_model(cfg, fuzz):
    pk = PACKETS + fuzz[:384]
    want = M.compose(cfg, pk)
    res = G.TunnelBatchResult(tls_parser(cfg), G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    assert len(res.levels) == 1
    w, got = want["levels"][0][0]["tls"], res.levels[0][0].tls
    for k in flows.TLSDecoder.KEYS:
        assert w[k].tobytes() == got[k].tobytes(), k
    i = NAMES.index("two_hellos")
    t, recs, hellos, arena = res.TLS(i)
    assert int(t["nrec"]) == len(recs) == 2 and len(hellos) == 2 and res.TLS(NAMES.index("plain_tcp_port_80")) is None
    assert bytes(arena[int(hellos[1]["sni_pos"]):int(hellos[1]["sni_pos"]) + int(hellos[1]["sni_len"])]) == b"two.test"
    assert len(res.TLS(NAMES.index("record_short_4"))[1]) == 0
    assert res.SNIs() == M.snis(w) and (i, b"one.test") in res.SNIs() and len(res.SNIs()) > 50


def test_composition_with_a_vxlan_level_control_layers_and_dns():
    """One parser holding the tunnel, control, DNS and TLS layers: the TLS pass
    runs behind the DNS pass on every level's part."""
    c, cc, dc = dict(CASES), dict(CC.quirk_cases()[0]), dict(DC.quirk_cases()[0])
    pk = [TC.over_udp(TC.vxlan(c["hello_with_sni"]), TC.VX), c["appdata_2"], cc["icmp4_echo"], dc["query_a"],
          TC.over_udp(TC.vxlan(c["sni_hostname_length_ffff_panics"]), TC.VX), c["plain_tcp_port_80"],
          TC.over_udp(TC.vxlan(c["length_one_short"]), TC.VX), TC.over_udp(TC.vxlan(dc["resp_soa"]), TC.VX)]
    cfg = dict(C.PARSER, tcp_port={8443: 140, 8080: 107})
    want = M.compose(cfg, pk, dns_on=True, control_kinds=15, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 20, 44, 140] and want["decoded"][1] == [17, 20, 44, 140]
    assert want["decoded"][2] == [17, 20, 19, 2] and want["decoded"][3] == [17, 20, 45, 107]
    assert want["error"][4] == "panic: runtime error: slice bounds out of range [9:8]" and not want["truncated"][4]
    assert want["error"][6] == "TLS packet length mismatch" and want["truncated"][6]
    assert want["decoded"][7] == [17, 20, 45, 116, 17, 20, 45, 107]
    p = tls_parser(cfg, extra=(L.TLS, L.DNS, L.ICMPv4, L.ICMPv6, L.ICMPv6Echo, L.ARP), tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._tunnels[2].VNI == 0x123456 and p._tls.Handshake[0].ClientHello.SNI == b"example.com"
    assert res.Hydrate(2, decoded) is None and p._controls[1].Id == 0x1234
    assert res.Hydrate(7, decoded) is None and p._dns.Answers[0].SOA.MName == b"ns.example.com"
    assert res.SNIs() == [(0, b"example.com")] and res.TLS(0)[2][0]["packet"] == 0


def test_inner_level_capacity_ends_with_the_inner_slice():
    """The scope decision of gpk_tls.h: on an inner tunnel level a ClientHello
    can read to the end of the inner slice, not into the bytes the outer
    packet holds behind it."""
    inner = C.over(C.cut_hello(50, sid=b"\xaa\xbb\xcc\xdd", ciphers=b"\x13\x01", comp=b"\x00"))
    pk = [TC.over_udp(TC.vxlan(inner), TC.VX, pad=6)]  # six bytes behind the IPv4 datagram
    p = tls_parser(C.PARSER, tunnels=(L.VXLAN,))
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    assert err_text(res.Err(0)) == "TLS ClientHello truncated in compression methods" and res.Truncated(0)


def test_snilist_example(tmp_path):
    """examples/snilist.py over a pcap of the cases: per name the packets and
    wire bytes of its ClientHellos, against the model."""
    pk = PACKETS + [golden_packet(v)[0] for v in GOLDEN] + [dict(CASES)["hello_with_sni"]] * 2
    path = tmp_path / "cases.pcap"
    with open(path, "wb") as f:
        f.write(struct.pack("<IHHiIII", 0xa1b2c3d4, 2, 4, 0, 0, 65535, 1))
        for i, p in enumerate(pk):
            f.write(struct.pack("<IIII", 1700000000 + i, 0, len(p), len(p) + 4) + p)  # four bytes more on the wire
    spec = importlib.util.spec_from_file_location("snilist", os.path.join(ROOT, "examples", "snilist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    got = mod.run(str(path), parser=tls_parser(), device=False, batch=40, log=lines.append)
    m, _ = decode_and_model(C.PARSER, pk)
    want = collections.OrderedDict()
    for i, name in M.snis(m):
        row = want.setdefault(name, [0, 0])
        row[0] += 1
        row[1] += len(pk[i]) + 4
    assert list(got.items()) == list(want.items()) and got[b"example.com"][0] >= 4 and b"www.google.com" in got
    assert len(lines) == len(want) and any("www.google.com" in ln for ln in lines)
