"""The IPv6 reassembly model (tests/defrag6_model.py) pinned on ip6defrag's own
test (defrag_test.go:17-67, from tests/golden/defrag6_testfrag.json), on the
quirks Q1-Q9 worked out by hand from defrag.go:82-178, on the keying rules of
include/gpk_defrag6.h and on the carry rule. Plus the C side of the header: it
compiles as C11 and C++, and its struct and constants match gopacket_amd/_lib.py.
CPU only; the device path is tests/test_defrag6_gpu.py."""
import ctypes
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest

import defrag6_model as M
import defrag6cases as DC
import pktutil
from configs import oracle_parser
from gopacket_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "IPV6_EXT", "TCP", "UDP", "PAYLOAD"])
CFG_NO_EXT = dict(first=17, decoders=["ETHERNET", "DOT1Q", "IPV4", "IPV6", "TCP", "UDP", "PAYLOAD"])
H = M.HELD


def run_model(packets, cfg=CFG, **kw):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(cfg).decode(data, off, cap, layouts=True)
    return M.run(packets, res["records"], res["layouts"], **kw)


def golden():
    with open(os.path.join(pktutil.GOLDEN, "defrag6_testfrag.json")) as f:
        return json.load(f)


def test_reference_testfrag_struct_level():
    """TestFrag literally: l1, l3, l2 give nil, nil, then the 24-byte payload."""
    g = golden()
    ip = SimpleNamespace(**{k: (bytes.fromhex(v) if isinstance(v, str) else v) for k, v in g["ipv6"].items()})
    frs = {k: SimpleNamespace(**{**v, "Payload": bytes.fromhex(v["Payload"])}) for k, v in g["fragments"].items()}
    d = M.IPv6Defragmenter()
    outs = [d.DefragIPv6(ip, frs[k]) for k in g["calls"]]
    assert [o is not None for o in outs] == g["returns"] == [False, False, True]
    out = outs[2]
    assert len(out.Payload) == 24 and out.NextHeader == 6 and out.Version == 6 and out.Length == 0
    for k, v in g["payload_checks"].items():
        assert out.Payload[int(k)] == v
    assert (out.Payload[0], out.Payload[15], out.Payload[16]) == (0x01, 0x18, 0x21)


def frames_of_testfrag():
    g = golden()
    fr = g["fragments"]
    return [DC.frag6(fr[k]["Identification"], fr[k]["FragmentOffset"], int(fr[k]["MoreFragments"]),
                     bytes.fromhex(fr[k]["Payload"]), nh=fr[k]["NextHeader"], src=bytes(16), dst=bytes(16), hlim=0)
            for k in g["calls"]]


def test_reference_testfrag_as_frames():
    r = run_model(frames_of_testfrag())
    assert r["verdict"] == [H, H, 0] and r["pending"] == [0, 1, 2]
    (d,) = r["datagrams"]
    assert d["length"] == 24 and d["nextheader"] == 6 and d["last"] == 2 and d["head"] == 0
    assert (d["payload"][0], d["payload"][15], d["payload"][16]) == (0x01, 0x18, 0x21)
    assert d["payload_off"] == 54 and d["data"][54:] == d["payload"]
    assert d["data"][14 + 4:14 + 6] == b"\x00\x18" and d["data"][14 + 6] == 6


@pytest.mark.parametrize("name", sorted(DC.quirk_cases()))
def test_quirks(name):
    pk, verdict, payloads = DC.quirk_cases()[name]
    r = run_model(pk)
    assert r["verdict"] == verdict
    assert [d["payload"] for d in r["datagrams"]] == payloads
    if name.startswith("Q3"):
        lay = r["datagrams"][0]["layer"]
        assert (lay.SrcIP, lay.DstIP, lay.HopLimit, lay.TrafficClass, lay.FlowLabel) == (DC.A, DC.B, 9, 3, 0x12345)
        assert lay.NextHeader == 6 and r["datagrams"][0]["head"] == 0
        d = r["datagrams"][0]["data"]
        assert d[14 + 8:14 + 24] == DC.A and d[14 + 7] == 9 and d[14 + 6] == 6
    if name.startswith("Q4"):
        assert r["datagrams"][0]["nextheader"] == 6
    if name.startswith("Q2"):
        assert r["pending"] == [0, 1, 3]  # ignored duplicates are not listed
    if name.startswith("Q9"):
        assert r["pending"] == [0, 1]


def test_keying_rules():
    p = b"k" * 8
    pk = [DC.frag6(1, 0, 1, p, front=(0, 60, 43)),              # behind HopByHop, Destination and Routing
          DC.frag6(1, 1, 0, p, front=(60,), vlan=3, behind=True, trailer=b"tr"),
          DC.frag6(2, 0, 1, p, front=(60,), cut=14 + 40 + 5),    # a short extension header
          DC.frag6(3, 0, 1, p, frag_bytes=7),                    # a 7-byte fragment header
          DC.frag6(4, 0, 1, p)[:20] + b"\x11" + DC.frag6(4, 0, 1, p)[21:],  # next header 17: no 44
          DC.frag6(5, 0, 1, p, front=(43,), length=8 + 4),       # Length ends inside the Fragment header
          DC.frag6(6, 0, 1, p, res=3)]                           # reserved bits beside M do not enter the offset
    r = run_model(pk)
    assert r["verdict"] == [H, 0, M.NONE, M.NONE, M.NONE, M.NONE, H]
    (d,) = r["datagrams"]
    # extension headers in front are dropped; the one behind the Fragment header is payload; the trailer is not
    assert d["payload"] == p + DC.ext(17, 60) + p and d["nextheader"] == 60 and d["payload_off"] == 54
    assert d["data"][:14] == pk[0][:14] and len(d["data"]) == 54 + 24
    assert r["lists"][6] == [6]
    # the same with and without IPV6_EXT in the parser
    r2 = run_model(pk, CFG_NO_EXT)
    assert r2["verdict"] == r["verdict"] and r2["pending"] == r["pending"]
    assert [x["data"] for x in r2["datagrams"]] == [x["data"] for x in r["datagrams"]]


def test_version_nibble_is_written_as_6():
    pk = [DC.frag6(1, 0, 1, b"v" * 8, version=5, tc=0xAB), DC.frag6(1, 1, 0, b"w" * 3, version=7)]
    r = run_model(pk)
    assert r["verdict"] == [H, 0]
    d = r["datagrams"][0]
    assert pk[0][14] >> 4 == 5 and d["data"][14] == 0x6A and d["data"][15] >> 4 == 0xB
    assert d["layer"].Version == 6 and d["layer"].TrafficClass == 0xAB


def test_truncated_capture_gives_fewer_bytes_and_big_payload_length_0():
    pk = [DC.frag6(1, 0, 1, b"t" * 16, cut=14 + 40 + 8 + 13), DC.frag6(1, 1, 0, b"u" * 8)]
    r = run_model(pk)
    assert r["verdict"] == [H, 0] and r["datagrams"][0]["payload"] == b"t" * 13 + b"u" * 8  # 13 / 8 == 1
    big = [DC.frag6(2, 0, 1, b"a" * 40000), DC.frag6(2, 5000, 0, b"b" * 25600)]
    d = run_model(big)["datagrams"][0]
    assert d["length"] == 65600 and d["data"][18:20] == b"\x00\x00"


def carry_sequence():
    p = [bytes([0x61 + k]) * 8 for k in range(6)]
    return [DC.frag6(1, 0, 1, p[0]), DC.frag6(2, 1, 0, p[1]), DC.frag6(1, 1, 0, p[2]), DC.frag6(1, 1, 0, p[3]),
            b"\x00" * 9, DC.frag6(2, 0, 1, p[4]), DC.frag6(1, 3, 0, p[5]), DC.frag6(3, 0, 0, p[0]),
            DC.frag6(2, 1, 0, p[1]), DC.frag6(3, 0, 0, p[1]), DC.frag6(1, 0, 1, p[2])]


def test_carry_reproduces_the_state_at_every_cut():
    pk = carry_sequence()
    whole = run_model(pk)
    assert len(whole["datagrams"]) == 7 and H in whole["verdict"]
    for cut in range(len(pk) + 1):
        a = run_model(pk[:cut])
        carried = [pk[i] for i in a["pending"]]
        b = run_model(carried + pk[cut:], carry=len(carried))
        assert b["verdict"][:len(carried)] == [M.CARRIED] * len(carried)
        got = [(cut + d["last"] - len(carried), d["data"]) for d in b["datagrams"]]
        assert [(d["last"], d["data"]) for d in a["datagrams"]] + got == \
            [(d["last"], d["data"]) for d in whole["datagrams"]], cut
        na = len(a["datagrams"])
        tail = [v if v < 0 else v + na for v in b["verdict"][len(carried):]]
        assert a["verdict"] + tail == whole["verdict"], cut
        # the lists are the whole run's, packet for packet
        back = a["pending"] + list(range(cut, len(pk)))
        assert {k: [back[i] for i in v] for k, v in b["lists"].items()} == whole["lists"], cut
    # without carry the replay itself would return datagrams a second time
    a = run_model(pk[:7])
    again = run_model([pk[i] for i in a["pending"]])
    assert len(again["datagrams"]) > 0


def test_header_compiles_as_c11_and_cxx(tmp_path):
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if not shutil.which(cc):
            pytest.skip("needs " + cc)
        src = tmp_path / ("hdr." + ext)
        src.write_text('#include "gpk_defrag6.h"\nint main(void) { gpk_datagrams6 d; (void)d; '
                       'return GPK_DEFRAG6_HELD + 32 + GPK_GROUP_DEFRAG6 - 4; }\n')
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                            str(tmp_path / "hdr.o"), str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_struct_and_constants_match_python(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    fields = [n for n, _ in _lib.Datagrams6._fields_]
    consts = dict(GPK_DEFRAG6_HELD=_lib.DEFRAG6_HELD, GPK_DEFRAG6_CARRIED=_lib.DEFRAG6_CARRIED,
                  GPK_DEFRAG6_MAX_LIST=_lib.DEFRAG6_MAX_LIST, GPK_GROUP_DEFRAG6=_lib.GROUP_DEFRAG6)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gpk_defrag6.h"', "int main(void) {",
             '  printf("{\\"size\\": %zu", sizeof(gpk_datagrams6));']
    lines += ['  printf(", \\"%s\\": %%zu", offsetof(gpk_datagrams6, %s));' % (f, f) for f in fields]
    lines += ['  printf(", \\"%s\\": %%d", (int)%s);' % (c, c) for c in consts]
    lines += ['  printf("}\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout)
    assert got.pop("size") == ctypes.sizeof(_lib.Datagrams6)
    for f in fields:
        assert got[f] == getattr(_lib.Datagrams6, f).offset, f
    for c, v in consts.items():
        assert got[c] == v, c
    assert (M.HELD, M.CARRIED, M.MAX_LIST, M.DEFRAG6) == (_lib.DEFRAG6_HELD, _lib.DEFRAG6_CARRIED,
                                                         _lib.DEFRAG6_MAX_LIST, _lib.GROUP_DEFRAG6)
