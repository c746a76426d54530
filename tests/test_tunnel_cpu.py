"""Tunnel decode without a GPU: the model (tunnel_model.py) against the pins
harvested from the reference's tests and the hand-derived quirk cases, then
gpk_tunnel_batch_host (the C++ the kernels run, on the calling thread) against
the model on every case and on the fuzz corpus, the composition through the
Python parser with the decode oracle in place of the device, Hydrate, the ABI
layout of gpk_tunnel and the level cap."""
import collections
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import configs
import tunnel_model as M
import tunnelcases as C
from gopacket_amd import _lib, flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import (GOLDEN, assert_same_peel, check_composition, err_text, golden_packet, model_and_host,
                        tunnel_parser)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, EXPECT = C.quirk_cases()


# ---- the model against the reference's own pins -------------------------------------
@pytest.mark.parametrize("v", GOLDEN, ids=[v["name"] for v in GOLDEN])
def test_model_reproduces_golden(v):
    cfg, pkt, shift = golden_packet(v)
    r = M.compose(cfg, [pkt])
    lvl0 = r["levels"][0][0]
    assert int(lvl0["peel"]["counts"][0]) == 1
    t = lvl0["peel"]["model"][0]
    e = v["expect"]
    if e.get("error"):
        assert t["err"] and bool(t["status"] & 1) == e["truncated"]
        assert r["error"][0] in ("GRE packet too small", "GRE packet truncated") and r["truncated"][0]
        return
    assert not t.get("err")
    assert [t["hdr_off"], t["hdr_off"] + t["contents_len"]] == [x + shift for x in e["Contents"]]
    assert [t["inner_off"], t["inner_off"] + t["inner_len"]] == [x + shift for x in e["Payload"]]
    if "layers" in v:  # the test's layer list, as far as this parser has decoders; then UnsupportedLayerType
        want = [x for x in v["layers"] if x != 113]
        n = len(r["decoded"][0])
        assert r["decoded"][0] == want[:n] and n == len(want) - 2
        assert r["error"][0] == "No decoder for layer type ICMPv4" and want[n] == 19
    if v["kind"] == "VXLAN":
        assert t["vni"] == e["VNI"] and t["gbp_id"] == e["GBPGroupPolicyID"]
        assert t["bits"] == (1 if e["ValidIDFlag"] else 0) | (2 if e["GBPExtension"] else 0) | \
            (4 if e["GBPDontLearn"] else 0) | (8 if e["GBPApplied"] else 0)
    elif v["kind"] == "Geneve":
        assert (t["gn_version"], t["gn_options_length"], t["protocol"], t["vni"]) == (
            e["Version"], e["OptionsLength"], e["Protocol"], e["VNI"])
        assert t["bits"] == (1 if e["OAMPacket"] else 0) | (2 if e["CriticalOption"] else 0)
        got = [dict(Class=o["Class"], Type=o["Type"], Length=o["Length"], Data=o["Data"].hex())
               for o in t.get("model_options", [])]
        assert got == e["Options"]
    else:
        assert t["protocol"] == e["Protocol"] and t["gre_checksum"] == e["Checksum"]
        assert bool(t["raw0"] & 0x80) == e["ChecksumPresent"]
        if "Valid" in e:  # TestGREChecksum: the serialized checksum verifies
            assert t["status"] & 2 and bool(t["status"] & 4) == e["Valid"] and t["gre_correct"] == e["Checksum"]
        else:
            assert (t["gre_key"], t["gre_seq"], t["gre_ack"]) == (e["Key"], e["Seq"], e["Ack"])


FIELD_OF = dict(contents="contents_len", inner="inner_len", next="next_type", err="err", a0="err_a0", a1="err_a1",
                bits="bits", count="count", version="gn_version", optlen="gn_options_length", csum="gre_checksum",
                off="gre_offset", key="gre_key", seq="gre_seq", ack="gre_ack", status="status")


def test_model_reproduces_hand_derived_quirks():
    pk = [p for _, p in CASES]
    data, offs, caps = pack(pk)
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    m = M.peel(C.PARSER, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"])
    cs = [int(x) for x in m["class_start"]]
    for i, (name, _) in enumerate(CASES):
        exp = EXPECT.get(name)
        if not exp:
            continue
        v = int(m["verdict"][i])
        assert v >= 0, name
        t = m["tunnels"][v]
        for k, want in exp.items():
            if k == "trunc":
                assert int(t["status"]) & 1 == want, name
            elif k == "cls":
                assert cs[want] <= v < cs[want + 1], (name, v, cs)
            else:
                assert int(t[FIELD_OF[k]]) == want, (name, k, int(t[FIELD_OF[k]]), want)
    for name in ("plain_tcp", "plain_udp_dns", "vxlan_empty_udp"):
        assert int(m["verdict"][[n for n, _ in CASES].index(name)]) == _lib.TUN_NONE


# ---- the host entry against the model --------------------------------------------------
def test_host_matches_model_on_golden_and_quirks():
    pk = [p for _, p in CASES] + [golden_packet(v)[1] for v in GOLDEN if golden_packet(v)[0] is C.PARSER or
                                  golden_packet(v)[0]["first"] == 17]
    for cfg in (C.PARSER, C.PARSER_IGNORE):
        m, h, _ = model_and_host(cfg, pk, fill=0xA5)
        assert_same_peel(m, h, "quirks")
        assert int(m["counts"][0]) >= len(CASES) - 3
    # a first layer other than Ethernet: TestDecodeGeneve1 behind its Linux SLL header
    v = [v for v in GOLDEN if v["name"] == "TestDecodeGeneve1"][0]
    cfg, pkt, _ = golden_packet(v)
    m, h, _ = model_and_host(cfg, [pkt])
    assert_same_peel(m, h, "sll")


@pytest.mark.parametrize("kinds", [1, 2, 4, 3, 5, 6])
def test_host_kinds_mask(kinds):
    m, h, _ = model_and_host(C.PARSER, [p for _, p in CASES], kinds=kinds)
    assert_same_peel(m, h, "kinds %d" % kinds)
    got = {int(t["kind"]) for t in h["tunnels"][:int(h["counts"][0])]}
    assert got and all(k & kinds for k in got)


def test_host_without_gre_checksum():
    m, h, _ = model_and_host(C.PARSER, [p for _, p in CASES], gre_checksum=False)
    assert_same_peel(m, h)
    assert int(h["counts"][7]) == 0 and not np.any(h["tunnels"][:int(h["counts"][0])]["status"] & 6)


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_packets(C.FUZZ_SEED, C.FUZZ_N)


def test_fuzz_corpus_covers_every_outcome(fuzz):
    """The model's results over the corpus contain every error code, every
    panic form and every class. GPK_TUN_ERR_GENEVE_OPT_SHORT (geneve.go:62) is
    the one site no input reaches: the walk enters with len >= OptionsLength +
    7, so before the uint8 offset wraps at least length - 1 >= 3 bytes are left,
    and after a wrap the offset is below 256 - 8 bytes into a slice longer than
    that; it is asserted absent, so a change that makes it reachable shows."""
    data, offs, caps = pack(fuzz)
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    m = M.peel(C.PARSER, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"])
    n = int(m["counts"][0])
    errs = collections.Counter(int(e) for e in m["tunnels"][:n]["err"])
    for code in (70, 71, 72, 74, 75, 76, 2, 3, 4):
        assert errs[code] > 0, (code, errs)
    assert errs[73] == 0
    assert all(int(c) > 0 for c in m["counts"][1:7]), m["counts"]
    assert int(m["counts"][7]) > 0 and np.count_nonzero(m["verdict"] == _lib.TUN_NONE) > 0


@pytest.mark.parametrize("align,pad", [(1, 0), (16, 3)])
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_host_matches_model_on_fuzz(fuzz, cfg, align, pad):
    m, h, _ = model_and_host(cfg, fuzz, align=align, pad=pad, fill=0xA5)
    assert_same_peel(m, h, "fuzz")


def test_table_edits_reach_the_host_entry():
    """UDP 8472 (the Linux kernel's VXLAN port) sent to LayerTypeVXLAN, and a
    private EtherType behind GRE sent to IPv4."""
    cfg = dict(C.PARSER, udp_port={8472: 116}, ethertype={0x9999: 20})
    ie = C.inner_eth()
    pk = [C.over_udp(C.vxlan(ie), 8472), C.over_ip(C.gre(ie[14:], 0x9999)), C.over_udp(C.vxlan(ie), 8473)]
    m, h, _ = model_and_host(cfg, pk)
    assert_same_peel(m, h)
    assert list(h["verdict"]) == [0, 1, _lib.TUN_NONE] and list(h["class_start"]) == [0, 1, 1, 2, 2, 2, 2]
    m0, h0, _ = model_and_host(C.PARSER, pk)
    assert_same_peel(m0, h0)
    assert int(h0["verdict"][0]) == _lib.TUN_NONE and int(h0["tunnels"][0]["next_type"]) == 0


def test_more_than_16_layers_is_unknown():
    pkt = C.MAC + b"".join(b"\x81\x00" + b"\x00\x05" for _ in range(14)) + b"\x08\x00" + C.ip4(
        C.udp(C.vxlan(C.inner_eth()), 50000, C.VX), 17)
    m, h, _ = model_and_host(C.PARSER, [pkt, C.over_udp(C.vxlan(C.inner_eth()), C.VX)])
    assert_same_peel(m, h)
    assert list(h["verdict"]) == [_lib.TUN_UNKNOWN, 0]


def test_host_argument_checks():
    p = configs.device_parser(C.PARSER)
    data, offs, caps = pack([CASES[0][1]])
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    for kinds in (0, 8):
        with pytest.raises(_lib.GpkError):
            flows.Detunneler.peel_host(data, offs, caps, ref["records"], ref["layouts"], p, kinds=kinds)
    out = flows.Detunneler.peel_host(data[:0], offs[:0], caps[:0], ref["records"][:0], ref["layouts"][:0], p)
    assert list(out["counts"]) == [0] * 8 and list(out["class_start"]) == [0] * 7


def test_format_error_texts():
    buf = ctypes.create_string_buffer(128)
    for code, a0, a1 in [(70, 0, 0), (71, 0, 0), (72, 0, 0), (73, 0, 0), (74, 0, 0), (75, 0, 0), (76, 0, 0), (2, 3, 3),
                         (3, 8, 7), (4, 8, 7)]:
        n = _lib.lib().gpk_tunnel_format_error(code, a0, a1, buf, 128)
        assert n == len(buf.value) and buf.value.decode() == M.error_text(code, a0, a1)
    assert _lib.lib().gpk_tunnel_format_error(10, 0, 0, buf, 128) == _lib.GPK_EINVAL


# ---- the ABI layout of gpk_tunnel and gpk_tunnels ----------------------------------------------
def test_abi_layout_of_tunnel_structs(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gpk_tunnel.h"', "int main(void) {"]
    want = {}
    for cname, mirror in (("gpk_tunnel", _lib.TUNNEL_DTYPE), ("gpk_tunnels", _lib.Tunnels)):
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
    assert _lib.TUNNEL_DTYPE.itemsize == 72


# ---- composition through the Python parser, the decode oracle in place of the device -----------
@pytest.mark.parametrize("cfg", [C.PARSER, C.PARSER_IGNORE], ids=["plain", "ignore_unsupported"])
def test_composition_matches_model(cfg, fuzz):
    pk = [p for _, p in CASES] + fuzz[:512]
    want = M.compose(cfg, pk)
    assert len(want["levels"]) >= 3  # two nested levels: vxlan_in_gre, geneve_in_geneve
    p = tunnel_parser(cfg)
    res = G.TunnelBatchResult(p, G.PacketBatch.from_packets(pk), device=False)
    check_composition(res, want, len(pk))


def test_hydrate_golden_packets():
    p = tunnel_parser()
    gre, vx, gn = p._tunnels[1], p._tunnels[2], p._tunnels[4]
    for v in GOLDEN:
        if v.get("bare_header") or v["skip"]:
            continue
        pkt = bytes.fromhex(v["hex"])
        decoded = []
        err = p.DecodeLayers(pkt, decoded)
        e = v["expect"]
        assert err_text(err) == "No decoder for layer type ICMPv4" or "Valid" in e
        lay = dict(GRE=gre, VXLAN=vx, Geneve=gn)[v["kind"]]
        assert lay.LayerContents() == pkt[e["Contents"][0]:e["Contents"][1]]
        assert lay.LayerPayload() == pkt[e["Payload"][0]:e["Payload"][1]]
        if v["kind"] == "VXLAN":
            assert (lay.ValidIDFlag, lay.VNI, lay.GBPExtension, lay.GBPApplied, lay.GBPDontLearn, lay.GBPGroupPolicyID) == (
                e["ValidIDFlag"], e["VNI"], e["GBPExtension"], e["GBPApplied"], e["GBPDontLearn"], e["GBPGroupPolicyID"])
            assert lay.NextLayerType() == L.LayerTypeEthernet
        elif v["kind"] == "Geneve":
            assert (lay.Version, lay.OptionsLength, lay.OAMPacket, lay.CriticalOption, lay.Protocol, lay.VNI) == (
                e["Version"], e["OptionsLength"], e["OAMPacket"], e["CriticalOption"], e["Protocol"], e["VNI"])
            assert [dict(Class=o.Class, Type=o.Type, Length=o.Length, Data=o.Data.hex()) for o in lay.Options] == e["Options"]
            assert lay.NextLayerType() == L.LayerTypeEthernet
        else:
            assert (lay.Protocol, lay.ChecksumPresent, lay.Checksum) == (e["Protocol"], e["ChecksumPresent"], e["Checksum"])
            assert lay.GRERouting is None and (lay.Key, lay.Seq, lay.Ack) == (0, 0, 0)
            _, r = lay.VerifyChecksum()
            assert r.Valid and (not lay.ChecksumPresent or r.Correct == e["Checksum"])
        # the other structs hold their innermost instance
        if v["name"] == "TestPacketVXLAN":
            assert p._decoders[_lib.DEC_IPV4].SrcIP == bytes([192, 168, 203, 3])
            assert p._decoders[_lib.DEC_ETHERNET].SrcMAC == bytes.fromhex("00163e37f604")


def test_hydrate_gre_routing_and_geneve_option_walk():
    p = tunnel_parser()
    cases = dict(CASES)
    p.DecodeLayers(cases["gre_R_3_sres"], [])
    g, lst = p._tunnels[1], []
    sre = g.GRERouting
    while sre is not None:
        lst.append((sre.AddressFamily, sre.SREOffset, sre.SRELength, sre.RoutingInformation))
        sre = sre.Next
    assert lst == [(2, 0, 4, b"abcd"), (2, 4, 8, b"efghijkl"), (7, 0, 0, b"")] and g.RoutingPresent
    decoded = []
    p.DecodeLayers(cases["geneve_opts_248_plus_4"], decoded)
    gn = p._tunnels[4]
    assert [o.Length for o in gn.Options] == [128, 120, 100] and len(gn.LayerContents()) == 100
    assert gn.Options[2].Class == 0x3f00 and gn.Options[2].Type == 0x65  # the header's own bytes


def test_parser_refuses_at_the_level_cap():
    inner = C.inner_eth()
    for _ in range(G.MAX_TUNNEL_LEVELS):
        inner = C.over_udp(C.vxlan(inner), C.VX)
    p = tunnel_parser()
    decoded = []
    assert p.DecodeLayers(inner, decoded) is None and decoded.count(116) == G.MAX_TUNNEL_LEVELS
    with pytest.raises(G.TunnelLevelsExceeded, match="MAX_TUNNEL_LEVELS"):
        p.DecodeLayers(C.over_udp(C.vxlan(inner), C.VX), [])


def test_parser_without_tunnel_layers_is_unchanged():
    p = tunnel_parser(tunnels=())
    assert not p._tunnels and sorted(p._decoders) == list(range(1, 9))
    only_vx = tunnel_parser(tunnels=(L.VXLAN,))
    decoded = []
    err = only_vx.DecodeLayers(dict(CASES)["gre_plain"], decoded)
    assert [int(t) for t in decoded] == [17, 20] and err_text(err) == "No decoder for layer type GRE"


def test_parser_options_act_on_the_composed_result():
    """IgnorePanic: a tunnel decoder's panic propagates (GoPanic) instead of
    becoming an error value; IgnoreUnsupported: a tunnel's undecodable next type
    is not an error, a tunnel decoder's own error still is."""
    cases = dict(CASES)
    p = tunnel_parser()
    assert err_text(p.DecodeLayers(cases["geneve_len7_cap10"], [])) == \
        "panic: runtime error: slice bounds out of range [8:7]"
    p.IgnorePanic = True
    with pytest.raises(G.GoPanic, match=r"slice bounds out of range \[8:7\]"):
        p.DecodeLayers(cases["geneve_len7_cap10"], [])
    q = tunnel_parser(C.PARSER_IGNORE)
    decoded = []
    assert q.DecodeLayers(cases["geneve_unregistered"], decoded) is None and int(decoded[-1]) == 120
    assert err_text(q.DecodeLayers(cases["gre_len3"], decoded)) == "GRE packet too small" and q.Truncated
