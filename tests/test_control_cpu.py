"""ICMPv4 / ICMPv6 / ICMPv6Echo / ARP decode without a GPU: the model
(control_model.py) against the pins harvested from the reference's tests and
the hand-derived quirk cases, then gpk_control_batch_host (the C++ the kernels
run, on the calling thread) against the model on every case and on the seeded
corpus, the composition through the Python parser with the decode oracle in
place of the device, Hydrate, VerifyChecksum, error texts and the ABI layout of
gpk_control."""
import collections
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import configs
import control_model as M
import controlcases as C
from controlutil import (FIELD_OF, GOLDEN, assert_same_control, control_parser, decode_and_model, err_text,
                         model_and_host)
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import check_composition
import tunnelcases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, EXPECT = C.quirk_cases()
PACKETS = [p for _, p in CASES]


# ---- the model against the reference's own pins -------------------------------------
@pytest.mark.parametrize("v", GOLDEN, ids=[v["name"] for v in GOLDEN])
def test_model_reproduces_golden(v):
    pkt = bytes.fromhex(v["hex"])
    m, _ = decode_and_model(C.PARSER, [pkt])
    assert int(m["counts"][0]) == 1
    t, e = m["records"][0], v["expect"]
    assert int(t["kind"]) == dict(ICMPv4=1, ICMPv6=2, ARP=8)[v["kind"]] and int(t["hdr_off"]) == v["at"]
    assert not int(t["err"])
    if v["kind"] != "ARP":  # the captures' checksums are intact: the harvest's pin
        assert e["Valid"] and int(t["status"]) & 6 == 6
        assert (int(t["correct"]), int(t["checksum"])) == (e["Correct"], e["Actual"])
    if "TypeCode" in e:
        assert (int(t["typecode"]), int(t["checksum"])) == (e["TypeCode"], e["Checksum"])
        assert [int(t["hdr_off"]), int(t["payload_off"])] == e["Contents"]
        assert [int(t["payload_off"]), int(t["payload_off"]) + int(t["payload_len"])] == e["Payload"]
    if "Type" in e:
        assert int(t["typecode"]) >> 8 == e["Type"] and v["at"] == e["TypeAt"]
    # the test's layer list (the full decoder set): the same layers up to the control layer, and its next type
    r = M.compose(C.PARSER, [pkt])
    k = e["layers"].index(int(t["layer_types"][0]))
    assert r["decoded"][0][:k + 1] == [x for x in e["layers"][:k + 1] if x != 46]  # HopByHop is inside IPv6 here
    if len(e["layers"]) > k + 1 and e["layers"][k + 1] != 2:
        assert int(t["unsupported"]) == int(t["next_type"]) == e["layers"][k + 1]
        assert r["error"][0] == "No decoder for layer type " + L.LayerType(e["layers"][k + 1]).String()


def test_model_reproduces_hand_derived_quirks():
    m, _ = decode_and_model(C.PARSER, PACKETS)
    cs = [int(x) for x in m["class_start"]]
    for i, (name, _) in enumerate(CASES):
        exp = EXPECT.get(name)
        v = int(m["verdict"][i])
        if not exp:
            assert v == _lib.CTL_NONE, name
            continue
        assert v >= 0, name
        t = m["records"][v]
        for k, want in exp.items():
            if k == "cls":
                assert cs[want] <= v < cs[want + 1], (name, v, cs)
            elif k == "lts":
                assert [int(x) for x in t["layer_types"][:int(t["nlayers"])]] == want, name
            else:
                assert int(t[FIELD_OF[k]]) == want, (name, k, int(t[FIELD_OF[k]]), want)


# ---- the host entry against the model --------------------------------------------------
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_host_matches_model_on_golden_and_quirks(cfg):
    pk = PACKETS + [bytes.fromhex(v["hex"]) for v in GOLDEN] + list(C.layers17())
    m, h, _ = model_and_host(cfg, pk, fill=0xA5)
    assert_same_control(m, h, "quirks")
    assert int(m["counts"][0]) >= len(EXPECT) and all(int(x) for x in m["counts"][1:6])
    assert list(m["verdict"][-2:]) == [int(m["class_start"][1]) - 1, _lib.CTL_UNKNOWN]  # 16 layers decode, 17 do not


def test_payload_absent_from_the_parser():
    """Without gopacket.Payload in the parser the loop returns LayerTypePayload."""
    m, h, _ = model_and_host(C.PARSER_NOPAYLOAD, PACKETS)
    assert_same_control(m, h)
    t = h["records"][int(h["verdict"][[n for n, _ in CASES].index("icmp4_echo")])]
    assert int(t["nlayers"]) == 1 and int(t["unsupported"]) == 2
    t = h["records"][int(h["verdict"][[n for n, _ in CASES].index("arp_reply_padded_60")])]
    assert int(t["nlayers"]) == 1 and int(t["unsupported"]) == 2


@pytest.mark.parametrize("kinds", [1, 2, 4, 8, 3, 6, 11, 14])
def test_host_kinds_mask(kinds):
    """Each layer absent from `kinds`: its packets are no candidates; without
    ICMPv6Echo an echo message ends with UnsupportedLayerType(ICMPv6Echo)."""
    m, h, _ = model_and_host(C.PARSER, PACKETS, kinds=kinds)
    assert_same_control(m, h, "kinds %d" % kinds)
    n = int(h["counts"][0])
    got = {int(t["kind"]) for t in h["records"][:n]}
    assert got and all(k & kinds for k in got)
    if kinds & 2 and not kinds & 4:
        t = h["records"][int(h["verdict"][[x for x, _ in CASES].index("icmp6_echo_request")])]
        assert int(t["nlayers"]) == 1 and int(t["unsupported"]) == 132


def test_host_without_checksum():
    m, h, _ = model_and_host(C.PARSER, PACKETS, checksum=False)
    assert_same_control(m, h)
    n = int(h["counts"][0])
    assert int(h["counts"][5]) == 0 and not np.any(h["records"][:n]["status"] & 14) and not np.any(h["records"][:n]["sum_init"])


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


def test_fuzz_corpus_covers_every_outcome(fuzz):
    """The model's results over the corpus contain every error code, every
    class, every appended-list form, an Echo failing behind a decoded ICMPv6,
    both checksum verdicts and the missing network layer."""
    m, _ = decode_and_model(C.PARSER, fuzz)
    n = int(m["counts"][0])
    r = m["records"][:n]
    errs = collections.Counter(int(e) for e in r["err"])
    for code in (80, 81, 82, 83, 84):
        assert errs[code] > 0, (code, errs)
    assert all(int(c) > 0 for c in m["counts"][1:6]), m["counts"]
    forms = collections.Counter((tuple(int(x) for x in t["layer_types"][:int(t["nlayers"])]), int(t["unsupported"]) != 0)
                                for t in r)
    for f in [((), False), ((19,), False), ((19, 2), False), ((57,), False), ((57,), True), ((57, 2), False),
              ((57, 132), False), ((10,), False), ((10, 2), False), ((132,), False)]:
        assert forms[f] > 0, (f, forms)
    assert np.any((r["err"] == 82) & (r["nlayers"] == 1)) and np.any((r["err"] == 82) & (r["nlayers"] == 0))
    st = collections.Counter(int(s) & 14 for s in r["status"])
    assert st[2] > 0 and st[6] > 0 and st[8] > 0
    assert np.count_nonzero(m["verdict"] == _lib.CTL_NONE) > 0
    m2, _ = decode_and_model(C.PARSER_NOPAYLOAD, fuzz[:512])
    r2 = m2["records"][:int(m2["counts"][0])]
    assert np.any((r2["kind"] == 1) & (r2["unsupported"] == 2)) and np.any((r2["kind"] == 8) & (r2["unsupported"] == 2))


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_host_matches_model_on_fuzz(fuzz, cfg, align, pad):
    m, h, _ = model_and_host(cfg, fuzz, align=align, pad=pad, fill=0xA5)
    assert_same_control(m, h, "fuzz")


def test_table_edits_reach_the_host_entry():
    """The three private EtherTypes of the cases' parser lead nowhere in a parser without the edits."""
    c = dict(CASES)
    pk = [c["icmp6_no_network_layer"], c["icmp4_no_network_layer"], c["echo_in_front"], c["icmp4_echo"]]
    m, h, _ = model_and_host(C.PARSER, pk)
    assert_same_control(m, h)
    assert list(h["verdict"]) == [2, 0, 3, 1] and list(h["class_start"]) == [0, 2, 4, 4, 4]
    plain = dict(C.PARSER, ethertype=None)
    m0, h0, _ = model_and_host(plain, pk)
    assert_same_control(m0, h0)
    assert list(h0["verdict"]) == [_lib.CTL_NONE] * 3 + [0]


def test_host_argument_checks():
    p = configs.device_parser(C.PARSER)
    data, offs, caps = pack([PACKETS[0]])
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    for kinds in (0, 16):
        with pytest.raises(_lib.GpkError):
            flows.ControlDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], p, kinds=kinds)
    out = flows.ControlDecoder.decode_host(data[:0], offs[:0], caps[:0], ref["records"][:0], ref["layouts"][:0], p)
    assert list(out["counts"]) == [0] * 8 and list(out["class_start"]) == [0] * 5


def test_format_error_texts():
    buf = ctypes.create_string_buffer(128)
    for code, a0, a1 in [(0, 0, 0), (80, 0, 0), (81, 0, 0), (82, 0, 0), (83, 7, 0), (84, 27, 28), (84, 28, 526)]:
        n = _lib.lib().gpk_control_format_error(code, a0, a1, buf, 128)
        assert n == len(buf.value) and buf.value.decode() == M.error_text(code, a0, a1)
    assert buf.value.decode() == "ARP length 28 too short, 526 expected"
    assert _lib.lib().gpk_control_format_error(10, 0, 0, buf, 128) == _lib.GPK_EINVAL
    assert _lib.lib().gpk_control_format_error(80, 0, 0, buf, 8) == 7 and buf.value == b"ICMP la"


# ---- the ABI layout of gpk_control and gpk_controls ---------------------------------------------
def test_abi_layout_of_control_structs(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_control.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_control", _lib.CONTROL_DTYPE), ("gpk_controls", _lib.Controls)):
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
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.splitlines()}
    assert got == want
    assert _lib.CONTROL_DTYPE.itemsize == 64


def test_exports_and_constants():
    for name in ("gpk_controller_create", "gpk_controller_destroy", "gpk_control_batch", "gpk_control_batch_host",
                 "gpk_controller_set_sum_threshold", "gpk_control_format_error"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "gpk_control.h")).read()
    for cname, val in (("GPK_CTL_ICMP4", _lib.CTL_ICMP4), ("GPK_CTL_ICMP6", _lib.CTL_ICMP6),
                       ("GPK_CTL_ICMP6ECHO", _lib.CTL_ICMP6ECHO), ("GPK_CTL_ARP", _lib.CTL_ARP),
                       ("GPK_CTL_ST_NONET", _lib.CTL_ST_NONET), ("GPK_CTL_SUM_GROUP_BYTES", _lib.CTL_SUM_GROUP_BYTES),
                       ("GPK_LT_ICMPV6_ECHO", _lib.LT_ICMPV6_ECHO), ("GPK_LT_ICMPV6", _lib.LT_ICMPV6)):
        assert "#define %s %du" % (cname, val) in hdr or "#define %s %d\n" % (cname, val) in hdr, cname
    assert _lib.CTL_SUM_GROUP_BYTES == _lib.TUN_SUM_GROUP_BYTES
    assert (int(L.LayerTypeICMPv6), int(L.LayerTypeICMPv6Echo), int(L.LayerTypeARP), int(L.LayerTypeICMPv4)) == (57, 132, 10, 19)
    assert int(L.LayerTypeMLDv2MulticastListenerQuery) == 139 and int(L.LayerTypeICMPv6NeighborSolicitation) == 126


# ---- composition through the Python parser, the decode oracle in place of the device -----------
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE, C.PARSER_NOPAYLOAD],
                         ids=["plain", "ignore_unsupported", "no_payload_decoder"])
def test_composition_matches_model(cfg, fuzz):
    pk = PACKETS + fuzz[:512]
    want = M.compose(cfg, pk)
    res = G.TunnelBatchResult(control_parser(cfg), G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    assert len(res.levels) == 1
    assert_same_control(want["levels"][0][0]["control"], res.levels[0][0].control)


def tunnelled():
    c = dict(CASES)
    v6 = c["icmp6_echo_request"]
    return [TC.over_udp(TC.vxlan(v6), TC.VX), TC.over_udp(TC.geneve(c["arp_reply_padded_60"]), TC.GN),
            TC.over_ip(TC.gre(c["icmp4_echo"][14:])), c["icmp4_echo"], TC.over_udp(TC.vxlan(TC.inner_eth()), TC.VX),
            TC.over_udp(TC.vxlan(c["icmp6_neighbor_solicitation"]), TC.VX), c["plain_tcp"]]


def test_composition_with_tunnel_layers():
    """The pass runs on every level's part: a VXLAN level in front of ICMPv6 + Echo."""
    pk = tunnelled()
    want = M.compose(C.PARSER, pk, tunnel_kinds=7)
    assert want["decoded"][0] == [17, 20, 45, 116, 17, 21, 57, 132]
    assert want["decoded"][1] == [17, 20, 45, 120, 17, 10, 2] and want["decoded"][2] == [17, 20, 18, 20, 19, 2]
    assert want["error"][5] == "No decoder for layer type ICMPv6NeighborSolicitation"
    p = control_parser(C.PARSER, tunnels=(L.GRE, L.VXLAN, L.Geneve))
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))
    decoded = []
    assert res.Hydrate(0, decoded) is None and [int(t) for t in decoded] == want["decoded"][0]
    assert p._tunnels[2].VNI == 0x123456 and p._controls[4].Identifier == 0xbeef
    assert p._controls[2].VerifyChecksum()[1].Valid
    assert p._decoders[_lib.DEC_IPV6].NextHeader == 58  # the inner network layer


# ---- the Python API --------------------------------------------------------------------------
def test_decode_layers_hydrate_and_verify_checksum():
    p = control_parser()
    c = dict(CASES)
    i4, i6, echo, arp = p._controls[1], p._controls[2], p._controls[4], p._controls[8]
    decoded = []
    assert p.DecodeLayers(c["icmp4_echo"], decoded) is None
    assert [int(t) for t in decoded] == [17, 20, 19, 2] and not p.Truncated
    assert (i4.TypeCode, i4.TypeCode.Type(), i4.TypeCode.Code(), i4.Id, i4.Seq) == (0x0800, 8, 0, 0x1234, 7)
    assert i4.LayerContents() == c["icmp4_echo"][34:42] and i4.LayerPayload() == b"ping-payload"
    assert p._decoders[_lib.DEC_PAYLOAD].LayerContents() == b"ping-payload"
    err, r = i4.VerifyChecksum()
    assert err is None and r.Valid and r.Correct == r.Actual == i4.Checksum
    assert i4.NextLayerType() == G.LayerTypePayload and i4.LayerType() == L.LayerTypeICMPv4
    p.DecodeLayers(c["icmp4_bad_checksum"], decoded)
    err, r = i4.VerifyChecksum()
    assert err is None and not r.Valid and r.Actual == r.Correct ^ 0x0100

    assert p.DecodeLayers(c["icmp6_echo_request"], decoded) is None
    assert [int(t) for t in decoded] == [17, 21, 57, 132]
    assert (i6.TypeCode.Type(), i6.TypeCode.Code(), echo.Identifier, echo.SeqNumber) == (128, 0, 0xbeef, 3)
    assert i6.NextLayerType() == L.LayerTypeICMPv6Echo and echo.LayerPayload() == b"" and echo.LayerContents() == b""
    assert i6.LayerPayload() == struct_echo(0xbeef, 3) + b"abcdefgh"
    assert i6.VerifyChecksum()[1].Valid
    p.DecodeLayers(c["icmp6_echo_reply_bad_checksum"], decoded)
    err, r = i6.VerifyChecksum()
    assert err is None and not r.Valid and r.Actual == r.Correct ^ 1
    p.DecodeLayers(c["icmp6_no_network_layer"], decoded)
    err, r = i6.VerifyChecksum()
    assert err.Error() == M.NO_NETWORK and r == G.ChecksumVerificationResult()

    assert p.DecodeLayers(c["arp_reply_padded_60"], decoded) is None and [int(t) for t in decoded] == [17, 10, 2]
    a = c["arp_reply_padded_60"][14:]
    assert (arp.AddrType, arp.Protocol, arp.HwAddressSize, arp.ProtAddressSize, arp.Operation) == (1, 0x0800, 6, 4, 2)
    assert (arp.SourceHwAddress, arp.SourceProtAddress, arp.DstHwAddress, arp.DstProtAddress) == (
        a[8:14], a[14:18], a[18:24], a[24:28])
    assert arp.LayerContents() == a[:28] and arp.LayerPayload() == bytes(18)
    assert arp.CanDecode().Contains(L.LayerTypeARP)


def struct_echo(ident, seq):
    return ident.to_bytes(2, "big") + seq.to_bytes(2, "big")


def test_error_texts_equal_the_reference():
    p = control_parser()
    c = dict(CASES)
    want = {"icmp4_len7": "ICMP layer less then 8 bytes for ICMPv4 packet",
            "icmp6_len3": "ICMP layer less then 4 bytes for ICMPv6 packet",
            "icmp6_echo_3_bytes": "ICMP layer less then 4 bytes for ICMPv6 Echo",
            "echo_in_front_3_bytes": "ICMP layer less then 4 bytes for ICMPv6 Echo",
            "arp_len7": "ARP length 7 too short", "arp_one_byte_short": "ARP length 27 too short, 28 expected",
            "arp_sizes_exceed_slice": "ARP length 28 too short, 526 expected",
            "icmp6_neighbor_solicitation": "No decoder for layer type ICMPv6NeighborSolicitation",
            "icmp6_mld_query_payload_20": "No decoder for layer type MLDv1MulticastListenerQuery",
            "icmp6_mld_query_payload_21": "No decoder for layer type MLDv2MulticastListenerQuery"}
    for name, text in want.items():
        decoded = []
        assert err_text(p.DecodeLayers(c[name], decoded)) == text, name
        assert p.Truncated == (not text.startswith("No decoder")), name
    decoded = []
    p.DecodeLayers(c["icmp6_echo_3_bytes"], decoded)
    assert [int(t) for t in decoded] == [17, 21, 57]  # the ICMPv6 layer decoded; the Echo behind it failed
    q = control_parser(C.PARSER_IGNORE)
    assert q.DecodeLayers(c["icmp6_neighbor_solicitation"], decoded) is None and int(decoded[-1]) == 57
    assert err_text(q.DecodeLayers(c["arp_len7"], decoded)) == "ARP length 7 too short" and q.Truncated


def test_each_layer_absent_from_the_parser():
    c = dict(CASES)
    decoded = []
    p = control_parser(controls=(L.ICMPv6, L.ARP))
    assert err_text(p.DecodeLayers(c["icmp4_echo"], decoded)) == "No decoder for layer type ICMPv4"
    assert [int(t) for t in decoded] == [17, 20]
    assert err_text(p.DecodeLayers(c["icmp6_echo_request"], decoded)) == "No decoder for layer type ICMPv6Echo"
    assert [int(t) for t in decoded] == [17, 21, 57]
    p = control_parser(controls=(L.ICMPv4,))
    assert err_text(p.DecodeLayers(c["arp_request_42"], decoded)) == "No decoder for layer type ARP"
    assert err_text(p.DecodeLayers(c["icmp6_echo_request"], decoded)) == "No decoder for layer type ICMPv6"
    assert p.DecodeLayers(c["icmp4_echo"], decoded) is None


def test_parser_without_control_layers_is_unchanged():
    p = control_parser(controls=())
    assert not p._controls and not p._tunnels and sorted(p._decoders) == list(range(1, 9))
    with pytest.raises(ValueError, match="fields=True"):
        control_parser().DecodeBatch(G.PacketBatch.from_packets(PACKETS[:2]), fields=True)
