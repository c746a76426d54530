"""DNS decode without a GPU: the model (dns_model.py) against the pins harvested
from the reference's tests, the messages of test_dns.pcap and the hand-derived
cases, then gpk_dns_batch_host (the C++ the kernels run, on the calling thread)
against the model on every case and on the seeded corpus, byte for byte, the
capacity rules, argument faults, error texts, the ABI layout, and the
composition through the Python parser with the decode oracle in place of the
device: DecodeLayers, Hydrate, a VXLAN level, the control layers beside it."""
import collections
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import configs
import controlcases as CC
import dns_model as M
import dnscases as C
import tunnelcases as TC
from dnsutil import (GOLDEN, assert_same_dns, decode_and_model, dns_parser, err_text, golden_packet, model_and_host,
                     pcap_dns_frames)
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, EXPECT = C.quirk_cases()
PACKETS = [p for _, p in CASES]
NAMES = [n for n, _ in CASES]


def hydrated(pkt, parser=None):
    """(error, decoded types, the DNS struct) of DecodeLayers on one packet."""
    p = parser or dns_parser()
    decoded = []
    err = p.DecodeLayers(pkt, decoded)
    return err, [int(t) for t in decoded], p._dns


# ---- the model against the reference's own pins -------------------------------------
@pytest.mark.parametrize("v", GOLDEN, ids=[v["name"] for v in GOLDEN])
def test_model_and_hydrate_reproduce_golden(v):
    """Each harvested vector through the model and through DecodeLayers +
    Hydrate (the host entry): the error text or the values the Go test compares."""
    pkt, at = golden_packet(v)
    e = v["expect"]
    m, _ = decode_and_model(C.PARSER, [pkt])
    assert int(m["counts"][0]) == 1 and int(m["records"][0]["hdr_off"]) == at
    err, decoded, d = hydrated(pkt)
    t = m["records"][0]
    if e["error"]:
        text = M.error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"]))
        assert int(t["err"]) and e["contains"] in text
        assert err_text(err) == text and decoded[-1] != 107
        return
    assert not int(t["err"]) and err is None and decoded[-1] == 107
    rows = M.messages(m)[0][2]
    for key, sec in (("questions", d.Questions), ("answers", d.Answers), ("additionals", d.Additionals)):
        if key in e:
            assert len(sec) == e[key] and sum(r["section"] == dict(questions=0, answers=1, additionals=3)[key]
                                              for r in rows) == e[key]
    if "Value" in e:  # TestParseDNSTypeTXT
        assert d.Answers[0].TXTs == [e["Value"].encode()] and [r["count"] for r in rows if r["section"] == 1] == [1]
    if "ResponseCode" in e:
        assert int(d.ResponseCode) == int(t["response_code"]) == e["ResponseCode"]
    if "OPTs" in e:
        assert len(d.Additionals[0].OPT) == e["OPTs"]
    if "OPTCode" in e:
        assert d.Additionals[0].OPT[0].Code == e["OPTCode"] and d.Additionals[0].OPT[0].Data[:7] == b"OpenDNS"
    if "Target" in e:
        u = d.Answers[0].URI
        assert (u.Target, u.Priority, u.Weight) == (e["Target"].encode(), e["Priority"], e["Weight"])
    raw = bytes.fromhex(v["hex"])
    if "SignerName" in e:
        s = d.Answers[0].RRSIG
        assert (int(s.TypeCovered), s.Algorithm, s.Labels, s.OriginalTTL, s.Expiration, s.Inception, s.KeyTag) == (
            e["TypeCovered"], e["Algorithm"], e["Labels"], e["OriginalTTL"], e["Expiration"], e["Inception"], e["KeyTag"])
        assert s.SignerName == e["SignerName"].encode() and s.Signature == raw[-e["Tail"]:]
    elif "Tail" in e:
        k = d.Answers[0].DNSKEY
        assert (k.Flags, k.Protocol, k.Algorithm, k.PublicKey) == (e["Flags"], e["Protocol"], e["Algorithm"], raw[-e["Tail"]:])
    if "Name" in e:
        first = (d.Questions + d.Answers)[0]
        assert first.Name == e["Name"].encode() == rows[0]["name"]
    if "RDataName" in e:
        a = d.Answers[0]
        got = {2: a.NS, 5: a.CNAME, 12: a.PTR, 15: a.MX.Name, 33: a.SRV.Name, 6: a.SOA.MName, 35: a.NAPTR.Replacement,
               64: a.SVCB.Target, 65: a.SVCB.Target, 46: a.RRSIG.SignerName}[int(a.Type)]
        assert got == e["RDataName"].encode() == rows[0]["rname"]
    if "RDataName2" in e:
        assert d.Answers[0].SOA.RName == e["RDataName2"].encode() == rows[0]["rname2"]


def test_model_and_host_reproduce_the_capture_fixture():
    """The UDP messages of test_dns.pcap: the ID and, in message order,
    (section, name, type, class, TTL) of every entry against
    tests/golden/dns_capture_expect.json, which dnspython's parse of the same
    bytes wrote (tools/make_dns_capture_expect.py); the model and the host
    entry both. The capture's first message is the harvested
    testPacketDNSRegression."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "dns_capture_expect.json")))["frames"]
    frames = pcap_dns_frames()
    assert len(frames) == len(want) == 10 and [len(f) for f in frames] == [w["frame_bytes"] for w in want]
    assert frames[0].hex() == next(v["hex"] for v in GOLDEN if v["name"] == "testPacketDNSRegression")
    m, h, _ = model_and_host(C.PARSER, frames)
    for out in (m, h):
        assert int(out["counts"][1]) == len(frames)
        for (pkt_i, rec, rows), w in zip(M.messages(out), want):
            assert (pkt_i, int(rec["id"])) == (w["frame"], w["id"])
            got = [[r["section"], r["name"].decode(), r["type"], r["cls"], r["ttl"]] for r in rows]
            assert got == w["entries"], pkt_i


def test_model_reproduces_hand_derived_cases():
    m, _ = decode_and_model(C.PARSER, PACKETS)
    msgs = {i: (rec, rows) for i, rec, rows in M.messages(m)}
    for i, name in enumerate(NAMES):
        exp, v = EXPECT[name], int(m["verdict"][i])
        if not exp:
            assert v == _lib.DNS_NONE, name
            continue
        assert v >= 0, name
        t = m["records"][v]
        assert (int(t["err"]), int(t["err_a0"]), int(t["err_a1"])) == (exp["err"], exp.get("a0", 0), exp.get("a1", 0)), name
        assert int(t["status"]) == exp.get("status", 0), name
        assert (v >= int(m["class_start"][1])) == bool(exp["err"]), name
        if exp["err"]:
            assert t.tobytes()[16:] == bytes(48) and int(t["hdr_off"]) > 0, name  # everything else is 0
            continue
        rows = msgs[i][1]
        for key, field in (("names", "name"), ("rnames", "rname"), ("rnames2", "rname2"), ("counts", "count")):
            if key in exp:
                assert [r[field] for r in rows] == exp[key], (name, key, [r[field] for r in rows])
        if "rcode" in exp:
            assert int(t["response_code"]) == exp["rcode"], name
        if "ident" in exp:
            assert int(t["id"]) == exp["ident"], name
    assert {EXPECT[n]["err"] for n in NAMES if EXPECT[n]} >= set(M.ALL_ERRORS)  # one case per error code at least


# ---- the host entry against the model --------------------------------------------------
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_host_matches_model_on_cases_and_golden(cfg):
    pk = PACKETS + [golden_packet(v)[0] for v in GOLDEN] + pcap_dns_frames() + list(C.layers17())
    m, h, _ = model_and_host(cfg, pk, fill=0xA5)
    assert_same_dns(m, h, "cases")
    assert int(m["counts"][1]) > 40 and int(m["counts"][2]) > 40 and not int(m["counts"][3])
    assert list(m["verdict"][-2:]) == [int(m["class_start"][1]) - 1, _lib.DNS_UNKNOWN]  # 16 layers decode, 17 do not


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


def test_fuzz_corpus_covers_every_outcome(fuzz):
    """With the model alone: at least a quarter of the corpus decodes, at
    least a quarter fails, every error code occurs."""
    m, _ = decode_and_model(C.PARSER, fuzz)
    n = int(m["counts"][0])
    errs = collections.Counter(int(e) for e in m["records"][:n]["err"])
    assert int(m["counts"][1]) * 4 >= len(fuzz) and int(m["counts"][2]) * 4 >= len(fuzz), m["counts"]
    for code in M.ALL_ERRORS:
        assert errs[code] > 0, (code, errs)
    assert np.count_nonzero(m["verdict"] == _lib.DNS_NONE) > 0


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
def test_host_matches_model_on_fuzz(fuzz, align, pad):
    m, h, _ = model_and_host(C.PARSER, fuzz, align=align, pad=pad, fill=0xA5)
    assert_same_dns(m, h, "fuzz")


def test_table_edits_reach_the_host_entry():
    """TCP port 8080 is a DNS port only in a parser with the edit."""
    pk = [dict(CASES)["table_edited_port"], dict(CASES)["query_a"]]
    m, h, _ = model_and_host(C.PARSER, pk)
    assert_same_dns(m, h)
    assert list(h["verdict"]) == [0, 1]
    m0, h0, _ = model_and_host(dict(C.PARSER, tcp_port=None), pk)
    assert_same_dns(m0, h0)
    assert list(h0["verdict"]) == [_lib.DNS_NONE, 0]


# ---- capacities -------------------------------------------------------------------------------
def test_capacity_rules():
    """Exact fit, one short in each arena, zero capacities: a message is
    written whole or not at all, nothing is written at or past a capacity,
    counts names what is needed, and the retry helper gets everything."""
    pk = PACKETS[:24]
    full, (data, offs, caps, ref) = decode_and_model(C.PARSER, pk)
    need_rr, need_nb = flows.DNSDecoder.needed(full["counts"])
    assert (need_rr, need_nb) == (len(full["rrs"]), len(full["names"])) and need_rr > 20 and need_nb > 100
    assert not int(full["counts"][3]) and not np.any(full["records"][:int(full["counts"][0])]["status"] & 2)
    for rr_cap, name_cap in ((need_rr, need_nb), (need_rr - 1, need_nb), (need_rr, need_nb - 1), (0, need_nb),
                             (need_rr, 0), (0, 0), (need_rr // 2, need_nb // 2), (need_rr + 3, need_nb + 3)):
        m, h, _ = model_and_host(C.PARSER, pk, fill=0xA5, rr_cap=rr_cap, name_cap=name_cap)
        assert_same_dns(m, h, "caps %d %d" % (rr_cap, name_cap))
        short = rr_cap < need_rr or name_cap < need_nb
        assert int(h["counts"][3]) == int(short) and flows.DNSDecoder.needed(h["counts"]) == (need_rr, need_nb)
        ok = h["records"][:int(h["counts"][1])]
        assert bool(np.any(ok["status"] & _lib.DNS_ST_DROPPED)) == short
        kept = ok[(ok["status"] & _lib.DNS_ST_DROPPED) == 0]
        assert all(int(t["rr0"]) + int(t["nrr"]) <= rr_cap and int(t["name0"]) + int(t["name_bytes"]) <= name_cap
                   for t in kept)
        for t in kept:  # what was kept is what the full run wrote
            a, b = int(t["rr0"]), int(t["rr0"]) + int(t["nrr"])
            assert h["rrs"][a:b].tobytes() == full["rrs"][a:b].tobytes()
    p = configs.device_parser(C.PARSER)
    out = flows.DNSDecoder.decode_host_all(data, offs, caps, ref["records"], ref["layouts"], p, rr_cap=1, name_cap=1)
    assert not int(out["counts"][3]) and out["rrs"].tobytes() == full["rrs"].tobytes()
    assert out["names"].tobytes() == full["names"].tobytes()


def test_host_argument_checks():
    p = configs.device_parser(C.PARSER)
    data, offs, caps = pack(PACKETS[:2])
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    out = flows.DNSDecoder.decode_host(data[:0], offs[:0], caps[:0], ref["records"][:0], ref["layouts"][:0], p, 0, 0)
    assert list(out["counts"]) == [0] * 8 and list(out["class_start"]) == [0] * 3
    lib = _lib.lib()
    good = flows.DNSDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], p, 8, 64)
    rrs = np.zeros(8 * 96 + 8, np.uint8)
    b = _lib.Batch(data.ctypes.data, offs.ctypes.data, caps.ctypes.data, 2, data.size)
    r = _lib.Results(ref["records"].ctypes.data, None, None, ref["layouts"].ctypes.data)

    def call(**kw):
        a = dict(verdict=good["verdict"].ctypes.data, class_start=good["class_start"].ctypes.data,
                 index=good["index"].ctypes.data, records=good["records"].ctypes.data, counts=good["counts"].ctypes.data,
                 rrs=good["rrs"].ctypes.data, names=good["names"].ctypes.data, rr_cap=8, name_cap=64)
        a.update(kw)
        return lib.gpk_dns_batch_host(p.h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(_lib.Dnss(**a)))
    assert call() == 0
    for kw in (dict(verdict=None), dict(class_start=None), dict(index=None), dict(records=None), dict(counts=None),
               dict(rrs=None), dict(names=None), dict(rrs=rrs.ctypes.data + (4 if rrs.ctypes.data % 8 == 0 else
                                                                              8 - rrs.ctypes.data % 8 + 4)),
               dict(records=good["records"].ctypes.data + 4)):
        assert call(**kw) == _lib.GPK_EINVAL, kw
    assert call(rrs=None, rr_cap=0) == 0 and call(names=None, name_cap=0) == 0
    assert lib.gpk_dns_batch_host(None, ctypes.byref(b), ctypes.byref(r), None) == _lib.GPK_EINVAL


def test_format_error_texts():
    buf = ctypes.create_string_buffer(256)
    lib = _lib.lib()
    for code in (0,) + M.ALL_ERRORS:
        for a0, a1 in ((0, 0), (0x41, 14), (3, 48), (65535, 4000000000)):
            n = lib.gpk_dns_format_error(code, a0, a1, buf, 256)
            assert n == len(buf.value) and buf.value.decode() == M.error_text(code, a0, a1), code
    lib.gpk_dns_format_error(M.E_Q40, 0x41, 14, buf, 256)
    assert buf.value.decode() == "qname '0x40' - RFC 2673 unsupported yet (data=41 index=14)"
    lib.gpk_dns_format_error(M.E_OPT_MAL, 46, 48, buf, 256)
    assert buf.value.decode() == "Malformed DNSOPT record.  Length 46 < 48"
    for bad in (1, 89, 121, 255):
        assert lib.gpk_dns_format_error(bad, 0, 0, buf, 256) == _lib.GPK_EINVAL
    assert lib.gpk_dns_format_error(90, 0, 0, buf, 8) == 7 and buf.value == b"DNS pac"
    assert lib.gpk_dns_format_error(90, 0, 0, None, 8) == _lib.GPK_EINVAL


def test_abi_layout_of_dns_structs(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a C compiler (gcc, cc or clang): the build needs a host compiler too"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_dns.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_dns", _lib.DNS_DTYPE), ("gpk_dns_rr", _lib.DNS_RR_DTYPE), ("gpk_dnss", _lib.Dnss)):
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
    assert (_lib.DNS_DTYPE.itemsize, _lib.DNS_RR_DTYPE.itemsize) == (64, 96)


def test_exports_and_constants():
    for name in ("gpk_dns_decoder_create", "gpk_dns_decoder_destroy", "gpk_dns_batch", "gpk_dns_batch_host",
                 "gpk_dns_format_error"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "gpk_dns.h")).read()
    for cname, val in (("GPK_LT_DNS", _lib.LT_DNS), ("GPK_DNS_ST_TRUNCATED", _lib.DNS_ST_TRUNCATED),
                       ("GPK_DNS_ST_DROPPED", _lib.DNS_ST_DROPPED), ("GPK_DNS_CLASS_FAILED", _lib.DNS_CLASS_FAILED),
                       ("GPK_DNS_SEC_ADDITIONAL", _lib.DNS_SEC_ADDITIONAL)):
        assert re.search(r"#define %s %du?\s" % (cname, val), hdr), cname
    assert "GPK_DNS_ERR_SHORT = %d," % _lib.DNS_ERR_FIRST in hdr and int(L.LayerTypeDNS) == 107
    assert (int(L.DNSTypeHTTPS), int(L.DNSTypeURI), int(L.DNSClassAny), int(L.DNSOpCodeUpdate),
            int(L.DNSResponseCodeBadCookie)) == (65, 256, 255, 5, 23)


# ---- the Python API, the decode oracle in place of the device -----------------------------------
def test_decode_layers_and_hydrate_every_case():
    """DecodeLayers of every case: decoded list, error text, Truncated, and
    the hydrated struct against the model's message."""
    p = dns_parser()
    m, _ = decode_and_model(C.PARSER, PACKETS)
    msgs = {i: (rec, rows) for i, rec, rows in M.messages(m)}
    for i, (name, pkt) in enumerate(CASES):
        decoded = []
        err = p.DecodeLayers(pkt, decoded)
        v = int(m["verdict"][i])
        if v < 0:
            assert 107 not in [int(t) for t in decoded], name
            continue
        t = m["records"][v]
        assert err_text(err) == M.error_text(int(t["err"]), int(t["err_a0"]), int(t["err_a1"])), name
        assert p.Truncated == bool(int(t["status"]) & 1), name
        assert (int(decoded[-1]) == 107) == (not int(t["err"])), name
        if int(t["err"]):
            continue
        d, rows = p._dns, msgs[i][1]
        assert d.LayerContents() == pkt[int(t["hdr_off"]):int(t["hdr_off"]) + int(t["len"])] and d.LayerPayload() == b""
        entries = d.Questions + d.Answers + d.Authorities + d.Additionals
        assert [(e.Name, int(e.Type), int(e.Class)) for e in entries] == [(r["name"], r["type"], r["cls"]) for r in rows]
        assert (len(d.Questions), len(d.Answers), len(d.Authorities), len(d.Additionals)) == (
            d.QDCount, d.ANCount, d.NSCount, d.ARCount), name
        assert int(d.ResponseCode) == int(t["response_code"]) and d.ID == int(t["id"])


def test_hydrated_fields_of_the_typed_records():
    c = dict(CASES)
    _, decoded, d = hydrated(c["resp_soa"])
    assert decoded == [17, 20, 45, 107] and (d.QR, d.RD, d.RA, d.AA, d.TC, d.Z, int(d.OpCode)) == (
        True, True, True, False, False, 0, 0)
    s = d.Answers[0].SOA
    assert (s.MName, s.RName, s.Serial, s.Refresh, s.Retry, s.Expire, s.Minimum) == (
        b"ns.example.com", b"admin.example.com", 1, 2, 3, 4, 5)
    a = hydrated(c["resp_a"])[2].Answers[0]
    assert (a.IP, a.TTL, a.DataLength, a.Data, int(a.Class)) == (bytes([192, 0, 2, 1]), 300, 4, bytes([192, 0, 2, 1]), 1)
    assert hydrated(c["resp_txt"])[2].Answers[0].TXTs == [b"abc", b"", b"hello"]
    assert hydrated(c["resp_txt"])[2].Answers[0].TXT == b"\x03abc\x00\x05hello"
    assert hydrated(c["resp_mx"])[2].Answers[0].MX == L.DNSMX(10, b"mail.example.com")
    assert hydrated(c["resp_srv"])[2].Answers[0].SRV == L.DNSSRV(1, 2, 5060, b"sip.example.com")
    assert hydrated(c["resp_naptr"])[2].Answers[0].NAPTR == L.DNSNAPTR(100, 10, b"u", b"E2U+sip", b"!^.!", b"r.example.com")
    assert hydrated(c["resp_opt"])[2].Additionals[0].OPT == [L.DNSOPT(10, bytes(8)), L.DNSOPT(12, b"")]
    s = hydrated(c["resp_rrsig"])[2].Answers[0].RRSIG
    assert (s.SignerName, s.Signature, s.KeyTag, s.Expiration) == (b"example.com", b"signature-bytes", 4242, 1700000000)
    assert hydrated(c["resp_dnskey"])[2].Answers[0].DNSKEY == L.DNSKEY(257, 3, 13, bytes(range(32)))
    v = hydrated(c["resp_svcb"])[2].Answers[0].SVCB
    assert v == L.DNSSVCB(1, b"svc.example.com", [L.DNSSvcParam(1, b"\x02h2"), L.DNSSvcParam(3, b"\x01\xbb")])
    assert hydrated(c["resp_uri"])[2].Answers[0].URI == L.DNSURI(10, 1, b"https://example.com/")
    assert hydrated(c["resp_ns"])[2].Answers[0].NS == b"ns1.example.com"
    assert hydrated(c["resp_cname"])[2].Answers[0].CNAME == b"www.example.org"
    assert hydrated(c["resp_ptr"])[2].Answers[0].PTR == b"host.com"
    z = hydrated(c["data_length_0_typed"])[2].Answers
    assert [(r.MX, r.SOA, r.SVCB, r.Data) for r in z] == [(L.DNSMX(), L.DNSSOA(), L.DNSSVCB(), b"")] * 3
    assert int(hydrated(c["opt_extended_rcode_twice"])[2].ResponseCode) == 0x33
    d = hydrated(c["resp_all_sections"])[2]
    assert [len(x) for x in (d.Questions, d.Answers, d.Authorities, d.Additionals)] == [1, 2, 1, 1]
    assert d.CanDecode().Contains(L.LayerTypeDNS) and d.NextLayerType() == G.LayerTypePayload


def test_capture_decodes_with_and_without_the_layer():
    """test_dns.pcap: [Ethernet IPv4 UDP DNS] with the questions of the
    harvested vector when the parser holds layers.DNS, and [Ethernet IPv4 UDP]
    + UnsupportedLayerType(DNS) when it does not."""
    pkt = pcap_dns_frames()[0]
    err, decoded, d = hydrated(pkt)
    assert err is None and decoded == [17, 20, 45, 107]
    assert [(q.Name, int(q.Type)) for q in d.Questions] == [(b"picslife.ru", 1)] and d.ID == 63000
    assert [int(a.Type) for a in d.Additionals] == [41]
    p = dns_parser(extra=())
    assert p._dns is None and not p._controls and not p._tunnels and sorted(p._decoders) == list(range(1, 9))
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets([pkt]), device=False)  # the host path of DecodeLayers
    assert err_text(res.Err(0)) == "No decoder for layer type DNS" and res.DNS(0) is None
    assert [int(t) for t in res.Decoded(0)] == [17, 20, 45]
    with pytest.raises(ValueError, match="fields=True"):
        dns_parser().DecodeBatch(G.PacketBatch.from_packets(PACKETS[:2]), fields=True)


@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_composition_matches_model(cfg, fuzz):
    pk = PACKETS + fuzz[:384]
    want = M.compose(cfg, pk)
    res = G.TunnelBatchResult(dns_parser(cfg), G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    assert len(res.levels) == 1
    w, got = want["levels"][0][0]["dns"], res.levels[0][0].dns
    for k in ("verdict", "class_start", "index", "records", "counts"):
        assert w[k].tobytes() == got[k].tobytes(), k
    need_rr, need_nb = flows.DNSDecoder.needed(got["counts"])
    assert got["rrs"][:need_rr].tobytes() == w["rrs"].tobytes() and got["names"][:need_nb].tobytes() == w["names"].tobytes()
    i = NAMES.index("resp_soa")
    t, rrs, names = res.DNS(i)
    assert int(t["nrr"]) == len(rrs) == 2 and int(rrs[1]["type"]) == 6 and res.DNS(NAMES.index("plain_tcp")) is None
    assert len(res.DNS(NAMES.index("short_11"))[1]) == 0


def test_composition_with_a_vxlan_level_and_control_layers():
    """One parser holding the tunnel, control and DNS layers: the DNS pass runs
    behind the control pass on every level's part."""
    c, cc = dict(CASES), dict(CC.quirk_cases()[0])
    pk = [TC.over_udp(TC.vxlan(c["resp_soa"]), TC.VX), c["query_a"], cc["icmp4_echo"], TC.over_udp(TC.vxlan(cc["arp_request_42"]), TC.VX),
          TC.over_udp(TC.vxlan(c["qname_0x40"]), TC.VX), c["plain_tcp"], TC.over_udp(TC.vxlan(c["short_11"]), TC.VX)]
    want = M.compose(C.PARSER, pk, control_kinds=15, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 20, 45, 107] and want["decoded"][1] == [17, 20, 45, 107]
    assert want["decoded"][2] == [17, 20, 19, 2] and want["decoded"][3] == [17, 20, 45, 116, 17, 10]
    assert want["error"][4] == "qname '0x40' - RFC 2673 unsupported yet (data=41 index=14)" and not want["truncated"][4]
    assert want["error"][6] == "DNS packet too short" and want["truncated"][6]
    p = dns_parser(C.PARSER, extra=(L.DNS, L.ICMPv4, L.ICMPv6, L.ICMPv6Echo, L.ARP), tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._tunnels[2].VNI == 0x123456 and p._dns.Answers[0].SOA.MName == b"ns.example.com"
    assert res.Hydrate(2, decoded) is None and p._controls[1].Id == 0x1234
