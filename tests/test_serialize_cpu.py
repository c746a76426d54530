"""gpk_serialize (include/gpk_serialize.h) on the CPU: the model
(tests/serialize_model.py) against the reference's own serialization pins
(tests/golden/serialize_vectors.json, tools/harvest_serialize.py), then
gpk_serialize_batch_host and the numpy path of gopacket.SerializeBatch against
the model, byte for byte, on tests/serializecases.py."""
import ctypes
import ipaddress
import json
import os
import struct

import numpy as np
import pytest

import serialize_model as M
import serializecases as C
from gopacket_amd import _lib, gopacket as G
from gopacket_amd.flows import Serializer
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "serialize_vectors.json")))
OPTS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def decode_one(pkt, first):
    data = np.frombuffer(bytes(pkt) + bytes(64), np.uint8)
    off, cap = np.zeros(1, np.uint64), np.array([len(pkt)], np.uint32)
    r = O.OracleParser(first, C.DECODERS).decode(data, off, cap)
    f = O.extract_fields(data, off, r["layouts"]).view(_lib.FIELDS_DTYPE).reshape(-1)
    return r["layouts"][0], f[0]


def model_one(pkt, first, fix, csum, edit=None):
    lay, f = decode_one(pkt, first)
    if edit:
        edit(f)
    return M.serialize_packet(pkt, lay["start"], lay["end"], f, fix, csum)


# ---- the model against the reference's pins ---------------------------------
@pytest.mark.parametrize("vec", VEC["roundtrip"] + [VEC["hopbyhop0"]], ids=lambda v: v.get("name", "hopbyhop0"))
def test_model_roundtrip_vectors(vec):
    """testSerialization / testSerializationWithOpts: decode, serialize, the same bytes"""
    pkt = bytes.fromhex(vec["packet"])
    for fix, csum in vec["opts"]:
        st, _, _, out = model_one(pkt, vec["first"], fix, csum)
        assert st == 0 and out == pkt, (vec.get("name"), fix, csum, out.hex())


def _udp_source(v):
    """The packet whose decode gives the struct values of layers/tcpip_test.go:21-56,
    lengths and checksums 0: FixLengths and ComputeChecksums fill them in."""
    u = struct.pack(">HHHH", v["ports"][0], v["ports"][1], 8, 0)
    if "ip4" in v:
        a = v["ip4"]
        return 20, struct.pack(">BBHHHBBH", 0x45, 0, 28, 0, 0, a["ttl"], 17, 0) + ipaddress.ip_address(a["src"]).packed + \
            ipaddress.ip_address(a["dst"]).packed + u, 26
    a = v["ip6"]
    d = bytes.fromhex(v["destination"])
    return 21, struct.pack(">IHBB", 6 << 28, len(d) + 8, 60, a["hop_limit"]) + ipaddress.ip_address(a["src"]).packed + \
        ipaddress.ip_address(a["dst"]).packed + d + u, 40 + len(d) + 6


@pytest.mark.parametrize("vec", VEC["checksums"], ids=lambda v: v["name"])
def test_model_checksum_vectors(vec):
    """layers/tcpip_test.go: the UDP checksum out of SerializeLayers{FixLengths, ComputeChecksums}"""
    first, pkt, at = _udp_source(vec)
    st, _, _, out = model_one(pkt, first, 1, 1)
    assert st == 0 and len(out) == len(pkt)
    assert struct.unpack(">H", out[at:at + 2])[0] == vec["want"]


def test_model_zero_udp_checksum():
    """layers/udp_test.go:380-408: a folded 0 is written as 0xffff"""
    z = VEC["zero_udp"]
    pkt = struct.pack(">BBHHHBBH", 0x40, 0, 0, 0, 0, 0, 17, 0) + ipaddress.ip_address(z["src"]).packed + \
        ipaddress.ip_address(z["dst"]).packed + struct.pack(">HHHH", z["ports"][0], z["ports"][1], 0, 0)
    # the test's IPv4 has IHL 0 and Length 0, which does not decode: IHL 5 and Length 28 are what FixLengths writes
    src = bytes([0x45]) + pkt[1:2] + struct.pack(">H", 28) + pkt[4:24] + struct.pack(">H", 8) + pkt[26:]
    st, _, _, out = model_one(src, 20, 1, 1)
    assert st == 0 and struct.unpack(">H", out[26:28])[0] == z["want"] == 0xFFFF


def test_model_tcp_padding():
    """layers/tcp_test.go:55-70: one No-op pads to 32 bits under FixLengths; DataOffset is a floor division"""
    t = VEC["tcp_padding"]
    opts = bytes.fromhex(t["options"])
    hdr = bytearray(C.tcp(b"", opts + bytes(3)))
    pkt = C.ip4(bytes(hdr), 6)
    lay, f = decode_one(pkt, 20)
    f["tcp_opt_map"] = [1, 0, 0, 0, 0]  # the struct of the test: the No-op alone
    st, _, _, out = M.serialize_packet(pkt, lay["start"], lay["end"], f, 1, 0)
    assert st == 0 and (len(out) - 20) % t["multiple_of"] == 0 and len(out) - 20 == 24 and out[20 + 12] >> 4 == 6
    st, _, _, out = M.serialize_packet(pkt, lay["start"], lay["end"], f, 0, 0)
    assert st == 0 and len(out) - 20 == 21  # without FixLengths nothing pads


def test_model_quirks():
    """the quirks include/gpk_serialize.h and the issue list, on the cases that reach them"""
    b = C.build("cases")
    idx = {n: i for i, n in enumerate(b["names"])}

    def run(name, fix, csum):
        i = idx[name]
        o, c = int(b["offsets"][i]), int(b["caplens"][i])
        pkt = bytes(b["data"][o:o + c])
        return pkt, M.serialize_packet(pkt, b["layouts"][i]["start"], b["layouts"][i]["end"], b["fields"][i], fix, csum)

    pkt, (st, _, _, out) = run("tcp_mptcp_doff8", 1, 0)  # 12 option bytes become [30, 2]: 20 + 2 + 2 zeros
    assert st == 0 and out[34 + 20:34 + 24] == bytes([30, 2, 0, 0]) and out[34 + 12] >> 4 == 6
    pkt, (st, _, _, out) = run("tcp_mptcp_doff8", 0, 0)  # OptionLength stays 12, DataOffset stays 8
    assert st == 0 and out[34 + 20:34 + 22] == bytes([30, 12]) and out[34 + 12] >> 4 == 8 and len(out) == len(pkt) - 10
    pkt, (st, _, _, out) = run("ip4_nop_nop_eol_pad5", 0, 0)  # Padding is never written; IHL still says 7
    assert st == 0 and out[14] == 0x47 and out[34:38] == b"\x01\x01\x00\x00" and out[38:40] == pkt[42:44]
    pkt, (st, _, _, out) = run("ip4_nop_nop_eol_pad5", 1, 0)
    assert out[14] == 0x46
    pkt, (st, _, _, out) = run("tcp_eol_pad_doff7", 0, 1)  # non-zero Padding after End of options is kept
    assert st == 0 and out[34 + 20:34 + 28] == b"\x00" + b"\x5A" * 7
    pkt, (st, _, _, out) = run("tcp_eol_pad_doff7", 1, 1)  # one option byte: FixLengths replaces it by 3 zeros
    assert st == 0 and out[34 + 20:34 + 24] == bytes(4) and out[34 + 12] >> 4 == 6 and len(out) == len(pkt) - 4
    pkt, (st, _, _, out) = run("tcp_3nop_eol_pad4", 1, 1)  # four option bytes: FixLengths keeps the Padding
    assert st == 0 and out[34 + 20:34 + 28] == b"\x01\x01\x01\x00" + b"\x5A" * 4 and out[34 + 12] >> 4 == 7
    pkt, (st, _, _, out) = run("hbh_pad1", 1, 0)  # Pad1 is written as 00 00; the pad is length % 8: 12 bytes, an error
    assert st == M.ERR_HBH_MULT8
    pkt, (st, _, _, out) = run("ip6_hbh_grow_ok", 0, 0)  # 8 Pad1 as 16 bytes: 24 bytes, HeaderLength still 1
    assert st == 0 and len(out) == len(pkt) + 8 and out[54 + 1] == 1 and out[54 + 2:54 + 18] == bytes(16)
    pkt, (st, _, _, out) = run("ip6_hbh_grow_ok", 1, 0)
    assert st == 0 and out[54 + 1] == 2 and struct.unpack(">H", out[18:20])[0] == 124
    pkt, (st, _, _, out) = run("ip4_wide_tcp_70000", 1, 0)  # Length = uint16(len): wraps
    assert st == 0 and len(out) == len(pkt) and struct.unpack(">H", out[16:18])[0] == (70000 + 40) & 0xFFFF
    pkt, (st, _, _, out) = run("ip4_tso_tcp_70000", 0, 0)  # the struct's Length is the slice's: not 0
    assert struct.unpack(">H", out[16:18])[0] == (70000 + 40) & 0xFFFF and pkt[16:18] == b"\0\0"
    assert len(out) == 14 + ((70000 + 40) & 0xFFFF)  # and the IPv4 decode trimmed the payload to it (ip4.go:203-204)
    pkt, (st, a0, _, out) = run("ip6_wide_udp_70000", 0, 0)
    assert (st, a0) == (M.ERR_IP6_FIT_LEN, 70008)
    assert run("ip6_wide_udp_70000", 1, 1)[1][0] == M.EJUMBOADD  # no HopByHop to carry the jumbo length
    # UDP's jumbo Length (udp.go:62-81) behind an IPv6 header that has its jumbo option: Length 0, the TLV filled
    # with the payload length (HopByHop included), and the pseudo-header's length summed in both halves
    pkt, (st, _, _, out) = run("ip6_jumbo_udp_70000", 1, 1)
    assert st == 0 and len(out) == len(pkt) == 14 + 40 + 8 + 8 + 70000
    assert out[18:20] == b"\0\0" and out[20] == 0 and struct.unpack(">I", out[58:62])[0] == 70016
    assert out[62 + 4:62 + 6] == b"\0\0"
    seg = out[62:]
    assert C.csum16(out[22:54] + struct.pack(">II", len(seg), 17) + seg) == 0 and len(seg) >> 16 == 1
    pkt, (st, _, _, out) = run("ip6_jumbo_udp_70000", 0, 1)  # without FixLengths the fields' lengths and the TLV stay
    assert st == 0 and out[18:20] == b"\x12\x34" and struct.unpack(">I", out[58:62])[0] == 99999
    assert struct.unpack(">H", out[62 + 4:62 + 6])[0] == 999
    seg = out[62:]
    assert C.csum16(out[22:54] + struct.pack(">II", len(seg), 17) + seg) == 0
    pkt, (st, _, _, out) = run("ip6_wide_udp_65535", 1, 0)  # 65 543 bytes behind IPv6: the same
    assert st == M.EJUMBOADD
    pkt, (st, _, _, out) = run("ip6_jumbo_70000", 1, 1)  # the 4-byte jumbo TLV is filled with the payload length
    assert st == 0 and struct.unpack(">I", out[54 + 4:54 + 8])[0] == len(out) - 54 and out[18:20] == b"\0\0"
    assert run("ip6_jumbo_notlv_70000", 0, 0)[1][0] == M.ERR_IP6_JUMBO_MISSING
    assert run("ip6_jumbo_notlv_70000", 1, 0)[1][0] == M.EJUMBOADD
    assert run("ip6_hbh_grow_fit", 1, 0)[1][0] == M.ERR_IP6_FIT
    assert run("hbh_32", 0, 0)[1][0] == M.EHBHLONG
    assert run("clear_ip4_keep_tcp", 0, 1)[1][0] == M.ERR_L4_NO_NETWORK and run("clear_ip4_keep_tcp", 1, 0)[1][0] == 0
    assert run("set_d1q_no_slice", 0, 0)[1][0] == M.ENOLAYER
    assert run("8023_type_conflict", 0, 0)[1][:3] == (M.ERR_ETH_TYPE_LENGTH, 0x0800, 50)
    assert run("eth_length_too_long", 0, 0)[1][:3] == (M.ERR_ETH_LENGTH, 0x0601, 0)
    pkt, (st, _, _, out) = run("vlan_pop", 1, 1)
    assert st == 0 and out[12:14] == b"\x08\x00" and len(out) == max(len(pkt) - 4, 60)
    pkt, (st, _, _, out) = run("dnat4", 1, 1)  # the rewrite reaches both checksums: the packet verifies
    assert out[30:34] == bytes([172, 16, 0, 99]) and C.csum16(out[14:34]) == 0
    assert C.csum16(out[26:34] + struct.pack(">HH", 6, len(out) - 34) + out[34:]) == 0
    pkt, (st, _, _, out) = run("sum_wraps_ff", 0, 1)  # the sum wraps mod 2^32 (checksum.go:35-50) before it folds
    body = out[34:34 + 16] + b"\0\0" + out[34 + 18:]
    n = len(body)
    want = M.fold_checksum((M.compute_checksum(out[26:34]) + 6 + (n & 0xFFFF) + (n >> 16) + M.compute_checksum(body)) & M.M32)
    assert struct.unpack(">H", out[34 + 16:34 + 18])[0] == want
    exact = sum(struct.unpack(">%dH" % (n // 2), body)) + sum(struct.unpack(">4H", out[26:34])) + 6 + (n & 0xFFFF) + (n >> 16)
    assert exact >> 32  # the premise: the exact sum does not fit 32 bits


def test_roundtrip_premise_c3():
    """decode -> serialize {} -> the same bytes for valid C3-style packets (the premise of the GPU round trip)"""
    from gopacket_amd import synth
    for cfg in (synth.C3_TCP1500, synth.C4_IMIX):
        d, o, c = synth.host_batch(cfg, 0, 256)
        lay, f = C.decode(d, o, c)
        ref = M.serialize_batch(d, o, c, lay, f, None, 0, 0)
        assert np.array_equal(ref["caplens"], c) and not ref["status"].any()
        for j in range(256):
            a, n = int(o[j]), int(c[j])
            assert bytes(ref["out"][int(ref["offsets"][j]):int(ref["offsets"][j + 1])]) == bytes(d[a:a + n])


# ---- the host path against the model ----------------------------------------
def same(got, ref, cap=None):
    assert np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["offsets"], ref["offsets"]) and np.array_equal(got["caplens"], ref["caplens"])
    assert np.array_equal(np.asarray(got["err_args"]).view(np.uint32), ref["err_args"])
    n = int(ref["counts"][1]) if cap is None else min(cap, int(ref["counts"][1]))
    assert np.array_equal(np.asarray(got["out"][:n]), ref["out"][:n])


@pytest.fixture(scope="module")
def ser():
    s = Serializer(device=None)
    yield s
    s.close()


@pytest.mark.parametrize("which", ["cases", "tails"])
@pytest.mark.parametrize("fix,csum", OPTS)
def test_host_matches_model(ser, which, fix, csum):
    b = C.build(which)
    ref = M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], None, fix, csum)
    got = ser.serialize_host(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], None, fix, csum)
    same(got, ref)
    if which == "cases":  # every status the cases are meant to reach is there
        want = {0, M.ENOLAYER, M.EHBHLONG, M.ERR_ETH_TYPE_LENGTH}
        want |= {M.EJUMBOADD, M.ERR_IP6_FIT} if fix else {M.ERR_IP6_JUMBO_MISSING, M.ERR_ETH_LENGTH, M.ERR_IP6_FIT_LEN}
        want |= {M.ERR_L4_NO_NETWORK} if csum else set()
        assert want <= set(int(x) for x in ref["status"])


def test_host_order_and_overflow(ser):
    b = C.build("cases")
    n = len(b["caplens"])
    rng = np.random.default_rng(5)
    small = np.nonzero(b["caplens"] < 4000)[0].astype(np.uint32)
    for order in (rng.permutation(small).astype(np.uint32), np.array([3, 3, 70, n, 3, 0, n + 5, 70], np.uint32),
                  np.zeros(0, np.uint32)):
        ref = M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], order, 1, 1)
        got = ser.serialize_host(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], order, 1, 1)
        same(got, ref)
    order = small[:40]
    full = M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], order, 1, 1)
    total = int(full["counts"][1])
    for cap in (0, int(full["offsets"][17]) + 1, total - 1):
        ref = M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], order, 1, 1, out_cap=cap)
        got = ser.serialize_host(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], order, 1, 1, out_cap=cap)
        assert int(ref["counts"][3]) == 1 and int(ref["counts"][0]) < 40
        assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["counts"], ref["counts"])
        assert np.array_equal(got["offsets"], ref["offsets"])
        for j in range(40):  # a packet that does not end inside cap is not written at all
            lo, hi = int(ref["offsets"][j]), int(ref["offsets"][j + 1])
            if hi <= cap:
                assert np.array_equal(got["out"][lo:hi], ref["out"][lo:hi])
            else:  # the output array started as zeros
                assert not got["out"][min(lo, cap):cap].any()


def test_numpy_path_and_errors():
    b = C.build("cases")
    res = G.SerializeBatch(G.SerializeOptions(FixLengths=True, ComputeChecksums=True), b["data"], b["offsets"],
                           b["caplens"], b["layouts"], b["fields"])
    ref = M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], None, 1, 1)
    same(res, ref)
    with pytest.raises(G.SerializeError) as e:
        G.SerializeBatch(G.SerializeOptions(), b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"],
                         raise_errors=True)
    j = int(np.nonzero(M.serialize_batch(b["data"], b["offsets"], b["caplens"], b["layouts"], b["fields"], None, 0, 0)
                       ["status"])[0][0])
    assert e.value.packet == j


def test_error_texts():
    """every reference error renders the reference's text (the cited lines of include/gpk_serialize.h)"""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    for st in range(1, 11):
        n = L.gpk_serialize_format_error(st, 70000, 77, buf, len(buf))
        want = M.error_text(st, 70000, 77)
        assert buf.value.decode() == want and n == len(want)
    assert L.gpk_serialize_format_error(0, 0, 0, buf, len(buf)) == 0
    assert L.gpk_serialize_format_error(_lib.SER_ENOLAYER, 0, 0, buf, len(buf)) == 0
    # %v of an EthernetType is its name
    assert G.SerializeError(_lib.SER_ERR_ETH_TYPE_LENGTH, 0x0800, 50).Error() == \
        "ethernet type IPv4 not compatible with length value 50"
    assert G.SerializeError(_lib.SER_ERR_IP6_FIT_LEN, 70000).Error() == "Cannot fit payload length of 70000 into IPv6 packet"
    assert str(G.SerializeError(_lib.SER_ERR_HBH_MULT8)) == "IPv6HopByHop actual length must be multiple of 8"
    # the texts are the reference's: read them where it has them
    assert M.ERR_ETH_LENGTH == _lib.SER_ERR_ETH_LENGTH and M.ELAYOUT == _lib.SER_ELAYOUT and M.EINDEX == _lib.SER_EINDEX


def test_abi_exports():
    L = _lib.lib()
    for name in ("gpk_serializer_create", "gpk_serializer_destroy", "gpk_serialize_batch", "gpk_serialize_batch_host",
                 "gpk_serialize_format_error"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.gpk_abi_version() == 2
    assert ctypes.sizeof(_lib.SerializeOpts) == 12
    h = ctypes.c_void_p()
    assert L.gpk_serializer_create(ctypes.byref(h), -1, 0) == 0  # host only
    cnt = np.zeros(4, np.uint64)
    off = np.ones(1, np.uint64)
    b = _lib.Batch(None, None, None, 0, 0)
    assert L.gpk_serialize_batch_host(h, ctypes.byref(b), None, None, None, 0, None, None, 0, off.ctypes.data, None,
                                      None, None, cnt.ctypes.data) == 0 and off[0] == 0
    assert L.gpk_serialize_batch(h, ctypes.byref(b), None, None, None, 0, None, None, 0, off.ctypes.data, None, None,
                                 None, cnt.ctypes.data, None) == _lib.GPK_EINVAL  # no device
    assert L.gpk_serializer_destroy(h) == 0


def test_bad_layouts_stay_inside_the_packet(ser):
    """layouts and maps that do not describe the packet are GPK_SER_ELAYOUT, and the model agrees"""
    b = C.build("cases")
    i = b["names"].index("tcp_mss_ts_doff10")
    lay, f = b["layouts"][i:i + 1].copy(), b["fields"][i:i + 1].copy()
    o, c = b["offsets"][i:i + 1], b["caplens"][i:i + 1]
    variants = []
    for k, (s, e) in enumerate(((2, 9), (40, 30), (int(c[0]) - 3, int(c[0]) + 50), (int(c[0]), 0xFFFFFFF0))):
        l2 = lay.copy()
        l2[0]["start"][C.IP4], l2[0]["end"][C.IP4] = s, e
        variants.append((l2, f))
    f2 = f.copy()
    f2[0]["tcp_opt_map"] = [0xFF] * 5
    variants.append((lay, f2))
    f3 = f.copy()
    f3[0]["ip4_opt_map"] = [0xFF] * 5
    variants.append((lay, f3))
    l3 = lay.copy()
    l3[0]["start"][C.UDP], l3[0]["end"][C.UDP] = int(c[0]) - 8, int(c[0])  # a transport slice after the TCP one
    variants.append((l3, f))
    for l, ff in variants:
        ref = M.serialize_batch(b["data"], o, c, l, ff, None, 1, 1)
        got = ser.serialize_host(b["data"], o, c, l, ff, None, 1, 1)
        same(got, ref)
        assert int(ref["status"][0]) == M.ELAYOUT
