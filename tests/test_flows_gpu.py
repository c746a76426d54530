"""gpk_group_batch (flow-keyed grouping in HBM) against the grouping oracle
(oracle/flows_oracle.py) run on the decode oracle's results: the same groups
in the same order, the same packets in each, the same reason codes, on
ip4defrag's test frames, tcpassembly's filter cases, fuzzed and golden
packets and C6 traffic; at 8 M packets, properties the grouping must have.
Then both entry points on batches that are not packed and ascending, at
offsets past 4 GiB, at sizes around a wave and a block with all, none and
some packets keyed, on one grouper used for many calls, and the GPK_EINVAL
contract (tests/flowcheck.py holds the comparison with the oracle)."""
import numpy as np
import pytest

import flowcases
import pktutil
from configs import CONFIGS, device_parser, oracle_parser
from flowcheck import DEFRAG6, Decoded, check_fused, check_group
from gopacket_amd import flows, synth
from oracle import flows_oracle as FO

pytestmark = pytest.mark.gpu

KINDS = [(FO.CONNECTION, 8), (FO.DEFRAG, 8), (FO.NET_BUCKET, 8), (FO.NET_BUCKET, 1024)]


def device_decode(gpu_ctx, data, off, cap, cfg):
    import torch
    n = off.numel()
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(device_parser(cfg), data, off, cap, rec, err, fl, lay, stream=torch.cuda.current_stream())
    return rec, fl, lay


def check(gpu_ctx, packets, cfg=flowcases.DEFRAG_PARSER, kinds=KINDS):
    import torch
    data, off, cap = pktutil.pack(packets)
    d = torch.from_numpy(data).cuda()
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    c = torch.from_numpy(cap.astype(np.int32)).cuda()
    rec, fl, lay = device_decode(gpu_ctx, d, o, c, cfg)
    ref = oracle_parser(cfg).decode(data, off, cap, layouts=True)
    g = flows.Grouper(max(len(packets), 1))
    for kind, buckets in kinds:
        out = g.group(d, o, c, rec, lay, fl, kind=kind, buckets=buckets)
        torch.cuda.synchronize()
        groups, group_of = flows.Grouper.to_lists(out)
        og, oc = FO.group(kind, packets, ref["records"], ref["layouts"], ref["flows"], buckets)
        assert group_of == oc, (kind, [(i, a, b) for i, (a, b) in enumerate(zip(group_of, oc)) if a != b][:5])
        assert groups == list(og.values()), kind
        first = out["first"][:len(groups)].cpu().tolist()
        assert first == [v[0] for v in og.values()]
        if kind in (FO.CONNECTION, FO.DEFRAG):  # the fused path: keys derived in the decode kernel
            n = len(packets)
            rec2 = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            fl2 = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
            out2 = g.decode_group(gpu_ctx, device_parser(cfg), d, o, c, rec2, None, fl2, kind=kind)
            torch.cuda.synchronize()
            groups2, group_of2 = flows.Grouper.to_lists(out2)
            assert group_of2 == oc and groups2 == groups, ("fused", kind)
            assert torch.equal(rec2, rec) and torch.equal(fl2, fl)
    g.close()


def test_defrag_frames_and_security_checks(gpu_ctx):
    frames, _ = flowcases.defrag_frames()
    pk = list(frames.values()) + [f for _, f in flowcases.defrag_struct_cases()] + list(frames.values())
    check(gpu_ctx, pk)


def test_connection_cases(gpu_ctx):
    check(gpu_ctx, flowcases.connection_cases() * 3)


def test_fuzzed_and_golden(gpu_ctx):
    pk = pktutil.fuzz_packets(91, 30000)
    for name in ("test_ethernet.pcap", "test_dns.pcap"):
        pk += pktutil.read_pcap(pktutil.GOLDEN + "/" + name)[1]
    check(gpu_ctx, pk)
    check(gpu_ctx, pk, cfg=CONFIGS["fragment_no_payload"])


def test_c6_traffic(gpu_ctx):
    data, off, cap = synth.host_batch(6, 1000, 200000)
    check(gpu_ctx, [bytes(data[o:o + c]) for o, c in zip(off, cap)])


def test_empty_and_single(gpu_ctx):
    check(gpu_ctx, [flowcases.connection_cases()[0]])
    check(gpu_ctx, [b"\x00" * 10])


def test_large_batch_properties(gpu_ctx):
    """8 M C6 packets generated in HBM: every group is one key (sampled against
    the oracle's key of its packets), groups are in first-appearance order,
    packets ascend inside a group, every keyed packet is in exactly one group."""
    import torch
    n = 8 << 20
    d, o, c = synth.device_batch(6, 0, n)
    cfg = flowcases.DEFRAG_PARSER
    rec, fl, lay = device_decode(gpu_ctx, d, o, c, cfg)
    g = flows.Grouper(n)
    out = g.group(d, o, c, rec, lay, fl, kind=FO.CONNECTION)
    torch.cuda.synchronize()
    G, K = out["counts"].cpu().tolist()
    perm = out["perm"][:K].cpu().numpy()
    start = out["start"][:G + 1].cpu().numpy()
    first = out["first"][:G].cpu().numpy()
    gof = out["group_of"].cpu().numpy()
    assert 0 < G < K <= n and start[0] == 0 and start[G] == K
    assert np.all(np.diff(first) > 0)                       # first appearance order
    assert np.array_equal(np.sort(perm), np.nonzero(gof >= 0)[0])  # a partition of the keyed packets
    gid = np.repeat(np.arange(G), np.diff(start))
    assert np.array_equal(gof[perm], gid)
    inner = np.diff(perm.astype(np.int64))
    assert np.all((inner > 0) | (np.diff(gid) > 0))         # ascending inside each group
    assert np.array_equal(perm[start[:-1]], first)
    # sampled groups: every packet's key (oracle, from the oracle decode) is the group's key
    rng = np.random.default_rng(3)
    seen = []
    for gg in list(rng.choice(G, 40, replace=False)) + [int(np.argmax(np.diff(start)))]:
        idx = perm[start[gg]:start[gg + 1]][:50]
        pk = [synth.packet(6, int(i)) for i in idx]
        data, off, cap = pktutil.pack(pk)
        ref = oracle_parser(cfg).decode(data, off, cap, layouts=True)
        keys = {FO.packet_key(FO.CONNECTION, p, ref["records"][k], ref["layouts"][k], 0, 8) for k, p in enumerate(pk)}
        assert len(keys) == 1 and not isinstance(next(iter(keys)), int)
        seen.append(next(iter(keys)))
    assert len(set(seen)) == len(seen)  # distinct groups, distinct keys
    g.close()


# ---------------------------------------------------------------------------
# batch layouts, offsets past 4 GiB, sizes, grouper reuse, argument contract

ALL_KINDS = KINDS + [(DEFRAG6, 8)]
FUSED = (FO.CONNECTION, FO.DEFRAG)


def edge_packets():
    pk = [p for _, p in flowcases.inline_boundary_cases() + flowcases.ip_in_ip_cases() +
          flowcases.useless_filter_cases()]
    pk += list(flowcases.defrag_frames()[0].values()) + [f for _, f in flowcases.defrag_struct_cases()]
    return pk + flowcases.connection_cases() + [p for _, p in flowcases.window_connection6()[::7]]


@pytest.mark.parametrize("layout", ["sparse4k", "sparse_mix", "gapped", "shuffled", "reversed", "wave_shuffled"])
def test_batch_layouts(gpu_ctx, layout):
    """Both entry points on batches that are not packed and ascending (what a
    tunnel level's in_offsets are): every kind through gpk_group_batch,
    CONNECTION and DEFRAG through gpk_decode_group_batch, whose records and
    flows equal a plain decode of the same batch."""
    from test_gpu_parity import golden_packets, phase_b_layout
    data, off, cap = phase_b_layout(pktutil.fuzz_packets(4242, 6000) + golden_packets() + edge_packets(), layout)
    packets = [bytes(data[int(o):int(o) + int(c)]) for o, c in zip(off, cap)]
    P = Decoded(gpu_ctx, packets, batch=(data, off, cap))
    g = flows.Grouper(P.n)
    for kind, buckets in ALL_KINDS:
        check_group(g, P, kind, buckets, what=layout)
        if kind in FUSED:
            check_fused(g, P, kind, what=layout)
    assert len(P.oracle(DEFRAG6)[0]) > 0  # the batch has IPv6 fragments
    g.close()


def test_offsets_past_4_GiB(gpu_ctx):
    """The same packets at base (1 << 32) + 3 of a device buffer: gpk_group_batch,
    gpk_decode_group_batch and gpk_pack_batch give what they give at base 0."""
    import torch
    packets = pktutil.fuzz_packets(4242, 2000) + edge_packets()
    data, off, cap = pktutil.pack(packets)
    base = (1 << 32) + 3
    P0 = Decoded(gpu_ctx, packets)
    big = torch.zeros(base + len(data) + 4096, dtype=torch.uint8, device="cuda")
    big[base:base + len(data)] = P0.d
    P1 = Decoded(gpu_ctx, packets, device_batch=(big, P0.o + base, P0.c), share=P0)
    g = flows.Grouper(P0.n)
    for kind, buckets in ALL_KINDS:
        outs = [check_group(g, P, kind, buckets, what="base") for P in (P0, P1)]
        if kind in FUSED:
            outs += [check_fused(g, P, kind, what="base") for P in (P0, P1)]
        for o in outs[1:]:
            assert all(torch.equal(o[k], outs[0][k]) for k in ("group_of", "counts")), kind
    g.close()
    rng = np.random.default_rng(5)
    order = torch.from_numpy(rng.integers(0, P0.n, 3000).astype(np.int32)).cuda()
    a = flows.pack_batch(P0.d, P0.o, P0.c, order)
    b = flows.pack_batch(big, P1.o, P1.c, order)
    torch.cuda.synchronize()
    want = np.concatenate([np.frombuffer(packets[i], np.uint8) for i in order.cpu().tolist()])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for out_data in (a[0], b[0]):  # the wrapper's 16 spare bytes past the packets are not written
        assert np.array_equal(out_data[:len(want)].cpu().numpy(), want)
    del big, P1, b
    torch.cuda.empty_cache()


def sized_packets(kind, n, shape):
    """n packets for `kind`: "all" keyed (about n / 3 keys), "none" keyed, or
    "mixed": the first half keyed, the rest not (the last keyed packet is
    followed by unkeyed ones)."""
    keys = max(1, n // 3)

    def keyed(i):
        k = (i * 7) % keys
        src = (10, 3, k >> 8, k & 255)
        if kind == FO.DEFRAG:
            return flowcases.eth_ip4(src, (10, 3, 0, 1), 0x100 + k, 1, 0, 28, proto=17, payload=bytes([i & 255]) * 8)
        return flowcases.tcp_segment(src, (10, 3, 0, 1), 1000 + k, 80, 2 if i % 5 else 24, b"p" * (1 + i % 9))

    def unkeyed(i):
        if kind == FO.NET_BUCKET:
            return flowcases.MAC + b"\x08\x06" + bytes([i & 255]) * 28
        if kind == FO.DEFRAG:
            return flowcases.tcp_segment((10, 3, 0, 2), (10, 3, 0, 1), 1000 + i % 50, 80, 2)
        if i % 2:  # ACK-only without payload: GPK_GROUP_USELESS
            return flowcases.tcp_segment((10, 3, 0, 2), (10, 3, 0, 1), 1000 + i % 50, 80, 16)
        return flowcases.eth_ip4((10, 3, 0, 2), (10, 3, 0, 1), i & 0xFFFF, 1, 0, 28, proto=17, payload=b"u" * 8)

    cut = {"all": n, "none": 0, "mixed": (n + 1) // 2}[shape]
    return [keyed(i) if i < cut else unkeyed(i) for i in range(n)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_and_keyed_shapes(gpu_ctx, n):
    """Batch sizes around a wave and a block, in a grouper of exactly that size:
    all packets keyed, none keyed (counts [0, 0], start[0] 0), keyed packets
    followed by unkeyed ones. The outputs start poisoned; flowcheck.compare
    asserts group_of, perm[:K], start[:G + 1], first[:G], counts, and that
    perm[K:] is a permutation of the unkeyed packets."""
    g = flows.Grouper(n)
    for kind, buckets in KINDS[:3]:
        for shape in ("all", "none", "mixed"):
            P = Decoded(gpu_ctx, sized_packets(kind, n, shape))
            groups, codes, _ = P.oracle(kind, buckets)
            keyed = sum(c >= 0 for c in codes)  # the shape is what it claims to be
            assert keyed == {"all": n, "none": 0, "mixed": (n + 1) // 2}[shape], (kind, shape, keyed)
            out = check_group(g, P, kind, buckets, what=(n, shape))
            if shape == "none":
                assert out["counts"].cpu().tolist() == [0, 0] and int(out["start"][0]) == 0
            if kind in FUSED:
                check_fused(g, P, kind, what=(n, shape))
    g.close()


def test_one_grouper_many_calls(gpu_ctx):
    """One Grouper(1025), never re-created, for 1025 (its capacity), 1, 257 and
    1025 packets, every kind and both entry points in turn on workspace the
    call before left behind; the first call repeated at the end gives its
    first result."""
    import torch
    g = flows.Grouper(1025)
    fuzz = pktutil.fuzz_packets(606, 1025 - len(edge_packets())) + edge_packets()
    batches = [Decoded(gpu_ctx, fuzz), Decoded(gpu_ctx, [flowcases.connection_cases()[0]]),
               Decoded(gpu_ctx, sized_packets(FO.DEFRAG, 257, "mixed")),
               Decoded(gpu_ctx, sized_packets(FO.CONNECTION, 1025, "all"))]
    assert [P.n for P in batches] == [1025, 1, 257, 1025]
    first = check_group(g, batches[0], FO.CONNECTION, what="first")
    step = 0
    for rounds in range(2):
        for P in batches:
            for kind, buckets in ALL_KINDS:
                step += 1
                if kind in FUSED and step % 2:
                    check_fused(g, P, kind, what=step)
                else:
                    check_group(g, P, kind, buckets, what=step)
    for kind in FUSED:
        for P in batches:
            check_fused(g, P, kind, what="fused")
    again = check_group(g, batches[0], FO.CONNECTION, what="again")
    assert all(torch.equal(first[k], again[k]) for k in first)
    g.close()


def test_argument_contract(gpu_ctx):
    """Every misuse returns GPK_EINVAL and leaves the grouper usable."""
    import ctypes

    import torch
    from gopacket_amd import _lib

    def einval(f, *a, **kw):
        with pytest.raises(_lib.GpkError, match=r"\(%d\)" % _lib.GPK_EINVAL):
            f(*a, **kw)

    P = Decoded(gpu_ctx, flowcases.connection_cases()[:4])
    P5 = Decoded(gpu_ctx, flowcases.connection_cases()[:5])
    g = flows.Grouper(4)

    def fused(P, kind):
        rec = torch.zeros(P.n * 16, dtype=torch.uint8, device="cuda")
        return g.decode_group(gpu_ctx, P.parser, P.d, P.o, P.c, rec, None, None, kind=kind)

    misuses = [lambda: g.group(P5.d, P5.o, P5.c, P5.rec, P5.lay, P5.fl, kind=FO.CONNECTION),  # n = max_packets + 1
               lambda: fused(P5, FO.CONNECTION)]
    misuses += [lambda b=b: g.group(P.d, P.o, P.c, P.rec, P.lay, P.fl, kind=FO.NET_BUCKET, buckets=b)
                for b in (0, 3, 1 << 17)]
    misuses += [lambda k=k: g.group(P.d, P.o, P.c, P.rec, P.lay, P.fl, kind=k) for k in (0, 5, 99)]  # unknown kinds
    misuses += [lambda: g.group(P.d, P.o, P.c, P.rec, P.lay, None, kind=FO.NET_BUCKET),   # no flows
                lambda: g.group(P.d, P.o, P.c, P.rec, None, P.fl, kind=FO.CONNECTION),    # no layouts
                lambda: g.group(P.d, P.o, P.c, P.rec, None, P.fl, kind=FO.DEFRAG),
                lambda: fused(P, DEFRAG6), lambda: fused(P, FO.NET_BUCKET), lambda: fused(P, 0)]
    for k, f in enumerate(misuses):
        einval(f)
        check_group(g, P, FO.CONNECTION, what=("after misuse", k))
    check_fused(g, P, FO.CONNECTION, what="after misuses")
    g.close()
    for cap in (0, 1 << 28):
        h = ctypes.c_void_p()
        assert _lib.lib().gpk_grouper_create(ctypes.byref(h), 0, cap) == _lib.GPK_EINVAL and not h
        einval(flows.Grouper, cap)
    assert _lib.lib().gpk_grouper_create(None, 0, 8) == _lib.GPK_EINVAL
    assert _lib.lib().gpk_grouper_hashes(None, 0, None) == _lib.GPK_EINVAL
