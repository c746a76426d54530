"""gpk_defrag6_batch (IPv6 reassembly in HBM, include/gpk_defrag6.h) and the
GPK_GROUP_DEFRAG6 grouping against the reassembly model (tests/defrag6_model.py)
run on the decode oracle's results: the same group and verdict for every
packet, the same datagrams in the same order (last, head, length, payload_off,
every byte), the same pending list and counts. No tolerance anywhere."""
import functools

import numpy as np
import pytest

import defrag6_model as M
import defrag6cases as DC
import pktutil
from configs import device_parser, oracle_parser
from gopacket_amd import _lib, flows
from test_defrag6_cpu import CFG, CFG_NO_EXT, carry_sequence, frames_of_testfrag

pytestmark = pytest.mark.gpu
H = M.HELD


def upload(packets):
    import torch
    data, off, cap = pktutil.pack(packets)
    return (torch.from_numpy(data).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
            torch.from_numpy(cap.astype(np.int32)).cuda())


def device_decode(gpu_ctx, d, o, c, cfg=CFG):
    import torch
    n = max(o.numel(), 1)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(device_parser(cfg), d, o, c, rec, None, fl, lay, stream=torch.cuda.current_stream())
    return rec, lay


def model(packets, cfg=CFG, **kw):
    data, off, cap = pktutil.pack(packets)
    res = oracle_parser(cfg).decode(data, off, cap, layouts=True)
    r = M.run(packets, res["records"], res["layouts"], **kw)
    r["groups"] = M.group(packets, res["layouts"])
    return r


def device_defrag(gpu_ctx, packets, data_cap, guard=0, carry=0, cfg=CFG):
    """-> (host dict: verdict, last, head, length, payload_off, offsets, caplens, pending, counts, data, groups,
    group_of; device dict)"""
    import torch
    d, o, c = upload(packets)
    rec, lay = device_decode(gpu_ctx, d, o, c, cfg)
    n = len(packets)
    g = flows.Grouper(max(n, 1))
    df = flows.Defragmenter6(max(n, 1))
    groups = g.group(d, o, c, rec, lay, kind=flows.DEFRAG6)
    out_data = torch.full((data_cap + guard + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    out = df.defrag(d, o, c, rec, lay, groups, carry=carry, data_cap=data_cap, out_data=out_data)
    torch.cuda.synchronize()
    counts = out["counts"].cpu().tolist()
    D, P = counts[0], counts[1]
    host = dict(verdict=out["verdict"].cpu().tolist(), counts=counts, pending=out["pending"][:P].cpu().tolist(),
                data=out["data"].cpu().numpy())
    for k in ("last", "head", "length", "payload_off", "offsets", "caplens"):
        host[k] = out[k][:D].cpu().tolist()
    host["groups"], host["group_of"] = flows.Grouper.to_lists(groups)
    g.close()
    df.close()
    return host, out


def check(gpu_ctx, packets, ref=None, carry=0, cfg=CFG):
    ref = ref or model(packets, cfg, carry=carry)
    dg = ref["datagrams"]
    need = sum(len(d["data"]) for d in dg)
    got, out = device_defrag(gpu_ctx, packets, need, carry=carry, cfg=cfg)  # exactly the bytes needed
    mgroups, mcodes = ref["groups"]
    assert got["group_of"][:len(packets)] == mcodes
    assert got["groups"] == list(mgroups.values())
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got["verdict"], ref["verdict"])) if a != b]
    assert not bad and len(got["verdict"]) == len(ref["verdict"]), bad[:8]
    assert got["last"] == [d["last"] for d in dg]
    assert got["head"] == [d["head"] for d in dg]
    assert got["length"] == [d["length"] for d in dg]
    assert got["payload_off"] == [d["payload_off"] for d in dg]
    assert got["caplens"] == [len(d["data"]) for d in dg]
    assert got["offsets"] == [int(x) for x in np.cumsum([0] + [len(d["data"]) for d in dg])[:-1]]
    blob = got["data"]
    for j, d in enumerate(dg):
        mine = blob[got["offsets"][j]:got["offsets"][j] + got["caplens"][j]].tobytes()
        assert mine == d["data"], ("datagram", j, next(k for k in range(len(mine)) if mine[k] != d["data"][k]))
        assert mine[d["payload_off"]:] == d["payload"]
    assert np.all(blob[need:] == 0xA5)  # nothing at or past data_cap
    assert got["pending"] == ref["pending"]
    assert got["counts"] == [len(dg), len(ref["pending"]), need, 0]
    return ref, got, out


def test_reference_testfrag(gpu_ctx):
    ref, got, _ = check(gpu_ctx, frames_of_testfrag())
    assert got["verdict"] == [H, H, 0] and got["length"] == [24]
    at = got["offsets"][0] + got["payload_off"][0]
    assert (got["data"][at], got["data"][at + 15], got["data"][at + 16]) == (0x01, 0x18, 0x21)
    assert got["data"][got["offsets"][0] + 14 + 6] == 6


@pytest.mark.parametrize("name", sorted(DC.quirk_cases()))
def test_quirks(gpu_ctx, name):
    pk, verdict, payloads = DC.quirk_cases()[name]
    ref, got, _ = check(gpu_ctx, pk)
    assert got["verdict"] == verdict
    blob = got["data"]
    assert [blob[o + p:o + c].tobytes() for o, p, c in zip(got["offsets"], got["payload_off"], got["caplens"])] == \
        payloads


# A jumbogram's payload is not advanced past its HopByHop header (ip6.go:249-256), so with the HopByHop's
# Next Header 44 the walk reads the HopByHop header's own 8 bytes as the Fragment header: the Jumbo TLV's
# length is its Identification
JUMBO = (b"\x02" * 12 + b"\x86\xdd" + bytes.fromhex("6000000000000040") + DC.A + DC.B +
         bytes([44, 0, 0xC2, 4]) + (65536 + 108).to_bytes(4, "big") + b"j" * 100)


def test_keying_rules_with_and_without_ext_decoder(gpu_ctx):
    p = b"k" * 8
    pk = [DC.frag6(1, 0, 1, p, front=(0, 60, 43)), DC.frag6(1, 1, 0, p, front=(60,), vlan=3, behind=True, trailer=b"tr"),
          DC.frag6(2, 0, 1, p, front=(60,), cut=14 + 40 + 5), DC.frag6(3, 0, 1, p, frag_bytes=7),
          DC.frag6(4, 0, 1, p)[:20] + b"\x11" + DC.frag6(4, 0, 1, p)[21:], DC.frag6(5, 0, 1, p, front=(43,), length=12),
          DC.frag6(6, 0, 1, p, res=3), DC.frag6(7, 0, 1, b"v" * 8, version=5, tc=0xAB), DC.frag6(7, 1, 0, b"w" * 3),
          DC.frag6(8, 0, 1, b"t" * 16, cut=14 + 40 + 8 + 13), DC.frag6(8, 1, 0, b"u" * 8),
          JUMBO]
    for cfg in (CFG, CFG_NO_EXT):
        ref, got, _ = check(gpu_ctx, pk, cfg=cfg)
        assert got["verdict"] == [H, 0, M.NONE, M.NONE, M.NONE, M.NONE, H, H, 1, H, 2, H]
        assert list(ref["groups"][0])[-1] == ("frag6", 65536 + 108)
        assert got["data"][got["offsets"][1] + 14] == 0x6A


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 129])
def test_group_sizes_around_the_wave(gpu_ctx, k):
    rng = np.random.default_rng(k)
    fwd = DC.in_order(1, k, rng)
    rev = DC.in_order(2, k, rng)[::-1]
    ref, _, _ = check(gpu_ctx, fwd + rev)
    assert len(ref["datagrams"]) == (2 if k > 1 else 0)  # a key's first call only stores


def test_re_emission_crosses_a_wave_of_datagrams(gpu_ctx):
    """One key completes and then receives 70 more duplicates and fragments
    behind the final one: 71 datagrams, all the same bytes, from one key."""
    rng = np.random.default_rng(3)
    first = DC.in_order(9, 4, rng, per=24, last=13)
    more = []
    for j in range(70):
        more.append(first[j % 4] if j & 1 else DC.frag6(9, 100 + j, j % 3 == 0, DC.body(rng, 8 + j)))
    ref, got, _ = check(gpu_ctx, [b"\x07" * 5] + first + more)
    assert len(ref["datagrams"]) == 71 and len({d["data"] for d in ref["datagrams"]}) == 1
    assert got["counts"][2] == 71 * len(ref["datagrams"][0]["data"])


def test_interleaved_keys(gpu_ctx):
    rng = np.random.default_rng(11)
    keys = [DC.in_order(100 + q, 5, rng, per=24) for q in range(64)]
    pk = [keys[q][j] for j in range(5) for q in range(64)]  # 64 keys round-robin
    ref, _, _ = check(gpu_ctx, pk)
    assert len(ref["datagrams"]) == 64


def test_full_list_reversed(gpu_ctx):
    """Offsets 0..8191 with 8 bytes each, arriving reversed: every insert shifts
    the whole list, one datagram at the last packet; a duplicate gives a second."""
    rng = np.random.default_rng(2)
    fr = DC.in_order(10, M.MAX_LIST, rng, per=8, last=8)
    pk = fr[::-1] + [fr[77]]
    ref, got, _ = check(gpu_ctx, pk)
    assert got["verdict"][:-2] == [H] * (M.MAX_LIST - 1) and got["verdict"][-2:] == [0, 1]
    assert got["length"] == [65536, 65536] and got["head"] == [M.MAX_LIST - 1] * 2
    assert bytes(got["data"][18:20]) == b"\x00\x00" and len(got["pending"]) == M.MAX_LIST


FIRST = (8, 16, 24, 1448)
FINAL = (0, 1, 7, 8, 15, 16, 17, 1447)
HEADERS = {"plain": {}, "vlan": dict(vlan=5), "dest": dict(front=(60,)), "vlan_dest": dict(vlan=5, front=(60,))}


@pytest.mark.parametrize("hdr", sorted(HEADERS))
def test_alignment_and_size_sweep(gpu_ctx, hdr):
    """Two-fragment datagrams, every first/final size, each behind 0-15 junk
    packets of odd length, so the source and destination 16-byte phases take
    all their values."""
    rng = np.random.default_rng(5)
    pk, ident = [], 0
    for junk in range(16):
        for a in FIRST:
            for b in FINAL:
                pk += [DC.body(rng, 2 * j + 1 + junk) for j in range(junk)]
                ident += 1
                pk.append(DC.frag6(ident, 0, 1, DC.body(rng, a), **HEADERS[hdr]))
                pk.append(DC.frag6(ident, a // 8, 0, DC.body(rng, b), trailer=b"\x00" * (3 if junk & 1 else 0),
                                   **HEADERS[hdr]))
    ref, got, _ = check(gpu_ctx, pk)
    assert len(ref["datagrams"]) == 16 * len(FIRST) * len(FINAL)
    assert {o & 15 for o in got["offsets"]} == set(range(16))


def test_payload_past_16_bits(gpu_ctx):
    rng = np.random.default_rng(13)
    pk = [b"\x01" * 3, DC.frag6(1, 0, 1, DC.body(rng, 40000)), DC.frag6(1, 5000, 0, DC.body(rng, 25600))]
    ref, got, _ = check(gpu_ctx, pk)
    assert got["length"] == [65600] and got["caplens"] == [54 + 65600]
    assert bytes(got["data"][18:20]) == b"\x00\x00"


def test_redecode_datagrams(gpu_ctx):
    """The datagram batch decodes again with the statsassembly parser: records
    equal the decode oracle's on the same bytes, and every UDP datagram built
    with a correct checksum verifies over the whole reassembled payload."""
    import torch
    rng = np.random.default_rng(21)
    pk = []
    for q in range(40):
        src, dst = DC.A[:15] + bytes([1 + q]), DC.B
        l4 = DC.udp_segment(src, dst, 5000 + q, 6000, DC.body(rng, 300 + 97 * q))
        fr = DC.fragments(q, l4, 256, src, dst, **({"vlan": 9} if q & 1 else {}), **({"front": (60,)} if q & 2 else {}))
        pk += fr[::-1] if q % 3 == 0 else fr
    ref, got, out = check(gpu_ctx, pk)
    D = got["counts"][0]
    assert D == 40
    dd, do, dc = out["data"], out["offsets"][:D].contiguous(), out["caplens"][:D].contiguous()
    rec, _ = device_decode(gpu_ctx, dd, do, dc)
    torch.cuda.synchronize()
    recs = rec.cpu().numpy().view(_lib.RECORD_DTYPE)[:D]
    want = oracle_parser(CFG).decode(got["data"], np.array(got["offsets"], np.uint64),
                                     np.array(got["caplens"], np.uint32), layouts=True)["records"]
    for f in ("layers", "status", "ip4_csum", "l4_csum"):
        assert np.array_equal(recs[f], want[f]), f
    ok = (1 << 22) | (1 << 23) | (1 << 24)  # GPK_ST_L4_CSUM | GPK_ST_L4_VALID | GPK_ST_L4_UDP
    assert np.all(recs["status"] & ok == ok) and np.all(recs["status"] & 0x7F == 0)


def test_data_cap_overflow(gpu_ctx):
    """data_cap ending inside the fourth datagram: the flag is set, the needed
    bytes are right, a guard region behind the cap stays untouched, and the
    first three datagrams are whole."""
    rng = np.random.default_rng(8)
    pk = []
    for q in range(6):
        pk += DC.fragments(q, DC.body(rng, 900 + q), per=304)
    ref = model(pk)
    sizes = [len(d["data"]) for d in ref["datagrams"]]
    need = sum(sizes)
    cap = sum(sizes[:3]) + 77
    got, _ = device_defrag(gpu_ctx, pk, cap, guard=4096)
    assert got["counts"] == [6, len(pk), need, 1]
    blob = got["data"]
    assert np.all(blob[sum(sizes[:3]):] == 0xA5)
    for j in range(3):
        assert blob[got["offsets"][j]:got["offsets"][j] + sizes[j]].tobytes() == ref["datagrams"][j]["data"]
    assert got["verdict"] == ref["verdict"] and got["caplens"] == sizes


def stream(s, parts):
    """IPv6Defragmenter over `parts` -> (verdicts with global datagram numbers, [(last, head, length, bytes)])"""
    import torch
    seen, verdicts = [], []
    for part in parts:
        d, o, c = upload(part)
        out = s.defrag(d, o[:len(part)], c[:len(part)])
        torch.cuda.synchronize()
        blob = out["data"].cpu().numpy()
        base = len(verdicts)
        for j in range(out["datagrams"]):
            at, ln = int(out["offsets"][j]), int(out["caplens"][j])
            seen.append((base + int(out["last"][j]), int(out["length"][j]), blob[at:at + ln].tobytes()))
        verdicts += [v if v < 0 else v + len(seen) - out["datagrams"] for v in out["verdict"].cpu().tolist()]
    return verdicts, seen


def test_streaming_two_batches(gpu_ctx):
    """A sequence cut in two at every position: the same datagrams in the same
    order as from one batch; with drop_completed the model with the same rule."""
    pk = carry_sequence()
    whole = model(pk)
    assert len(whole["datagrams"]) == 7
    s = flows.IPv6Defragmenter(gpu_ctx, device_parser(CFG), 64)
    sd = flows.IPv6Defragmenter(gpu_ctx, device_parser(CFG), 64, drop_completed=True)
    for cut in range(len(pk) + 1):
        first = model(pk[:cut])
        verdicts, seen = stream(s, (pk[:cut],))
        assert s.pending_count == len(first["pending"])
        v2, seen2 = stream(s, (pk[cut:],))
        seen += [(cut + a, b, c) for a, b, c in seen2]
        verdicts += [v if v < 0 else v + len(first["datagrams"]) for v in v2]
        assert seen == [(d["last"], d["length"], d["data"]) for d in whole["datagrams"]], cut
        assert verdicts == whole["verdict"], cut
        assert s.pending_count == len(whole["pending"]) and s.flush() == len(whole["pending"])
        assert s.pending_count == 0
        # drop_completed: the keys that returned a datagram in the first call start again in the second
        a = model(pk[:cut], drop_completed=True)
        carried = [pk[i] for i in a["pending"]]
        b = model(carried + pk[cut:], carry=len(carried), drop_completed=True)
        va, sa = stream(sd, (pk[:cut],))
        assert sd.pending_count == len(carried)
        vb, sb = stream(sd, (pk[cut:],))
        assert va == a["verdict"] and vb == b["verdict"][len(carried):], cut
        assert [x[1:] for x in sb] == [(d["length"], d["data"]) for d in b["datagrams"]], cut
        assert [x[0] for x in sb] == [d["last"] - len(carried) for d in b["datagrams"]], cut
        assert sd.flush() == len(b["pending"])
    s.close()
    sd.close()


def test_streaming_head_from_a_carried_packet(gpu_ctx):
    import torch
    pk = DC.quirk_cases()["Q8 reversed"][0]
    s = flows.IPv6Defragmenter(gpu_ctx, device_parser(CFG), 16)
    d, o, c = upload(pk[1:])  # offsets 1, 0 | then the final fragment: the head is carried
    out = s.defrag(d, o[:2], c[:2])
    assert out["datagrams"] == 0 and s.pending_count == 2
    d, o, c = upload(pk[:1])
    out = s.defrag(d, o[:1], c[:1])
    torch.cuda.synchronize()
    assert out["datagrams"] == 1 and out["last"].cpu().tolist() == [0] and out["head"].cpu().tolist() == [-1]
    blob = out["data"].cpu().numpy()
    assert blob[:int(out["caplens"][0])].tobytes() == model([pk[1], pk[2], pk[0]])["datagrams"][0]["data"]
    s.close()


def test_streaming_re_emission_outgrows_the_batch(gpu_ctx):
    """A 3 KB datagram returned again by each of 40 small duplicates: the bytes
    needed are many times the batch's, and the streaming class sizes its data
    from the first attempt's count."""
    import torch
    rng = np.random.default_rng(17)
    big = [DC.frag6(5, 0, 1, DC.body(rng, 1448)), DC.frag6(5, 181, 1, DC.body(rng, 1448)),
           DC.frag6(5, 362, 0, DC.body(rng, 8))]
    pk = big + [big[2]] * 40
    whole = model(pk)
    need = sum(len(d["data"]) for d in whole["datagrams"])
    assert len(whole["datagrams"]) == 41 and need > 10 * sum(len(p) for p in pk)
    s = flows.IPv6Defragmenter(gpu_ctx, device_parser(CFG), 64)
    verdicts, seen = stream(s, (pk[:2], pk[2:]))
    assert verdicts == whole["verdict"] and s.pending_count == 3
    assert seen == [(d["last"], d["length"], d["data"]) for d in whole["datagrams"]]
    s.close()


@functools.lru_cache(maxsize=None)
def random_case():
    pk = DC.random_traffic(4, 3000, lo=2500, hi=7000, per=744)
    return pk, model(pk)


def test_random_traffic(gpu_ctx):
    pk, ref = random_case()
    v = ref["verdict"]
    assert 19000 < len(pk) < 23000
    assert len(ref["datagrams"]) >= 1500 and H in v
    mcodes = ref["groups"][1]
    returned = [mcodes[d["last"]] for d in ref["datagrams"]]
    assert len(returned) > len(set(returned))  # at least one key returned its datagram again
    check(gpu_ctx, pk, ref)


def test_fuzz_packets(gpu_ctx):
    pk = pktutil.fuzz_packets(91, 20000)
    ref, _, _ = check(gpu_ctx, pk)
    assert sum(c >= 0 for c in ref["groups"][1]) > 20


def test_edges(gpu_ctx):
    check(gpu_ctx, [DC.frag6(1, 0, 1, b"a" * 8)[:40], b"\x00" * 10])                 # no keyed packet
    check(gpu_ctx, [DC.frag6(1, 0, 1, b"a" * 8), DC.frag6(2, 0, 1, b"b" * 8)])       # keyed, no datagram
    import torch
    df = flows.Defragmenter6(4)
    z64, z32, z8 = (torch.zeros(1, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.uint8))
    groups = dict(group_of=z32, perm=z32, start=z32, first=z32, counts=torch.zeros(2, dtype=torch.int32, device="cuda"))
    out = df.defrag(z8, z64[:0], z32[:0], z8, z8, groups)
    torch.cuda.synchronize()
    assert out["counts"].cpu().tolist() == [0, 0, 0, 0]
    df.close()
    g = flows.Grouper(4)
    with pytest.raises(_lib.GpkError):  # the fused decode + grouping does not take DEFRAG6
        g.decode_group(gpu_ctx, device_parser(CFG), z8, z64, z32, torch.zeros(16, dtype=torch.uint8, device="cuda"),
                       kind=flows.DEFRAG6)
    g.close()
