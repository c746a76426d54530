"""The hash table of gpk_group_batch / gpk_decode_group_batch (insert_kernel)
where chance never takes it: different keys with an equal 36-bit tag in one
home slot (only the exact key comparison tells them apart), probe chains of
300 keys that wrap from the last slot to slot 0, 60 000 packets racing on one
slot word, and FastHash buckets on both sides of the 4096-bucket branch.

The keys are chosen by their hash through tests/grouphash.py, a numpy
restatement of the key words and the hash; test_restatement_holds pins it to
the device (Grouper.hashes, a test aid) and is the precondition of the rest.
Groups come from oracle/flows_oracle.py on the decode oracle's results, except
in the 60 000-packet test, which says where its groups come from."""
import numpy as np
import pytest

import flowcases
import grouphash as H
import pktutil
from flowcheck import Decoded, check_fused, check_group, compare, poisoned
from gopacket_amd import flows, synth
from oracle import flows_oracle as FO

pytestmark = pytest.mark.gpu

KIND = {"conn": FO.CONNECTION, "frag": FO.DEFRAG}


def packet_of(kind, c, salt=0):
    """The packet of grouphash candidate c: a SYN segment / a first fragment."""
    f = H.candidate(kind, c)
    if kind == "frag":
        return flowcases.eth_ip4(f["src"], f["dst"], f["ident"], 1, 0, 28, proto=17, payload=bytes([salt]) * 8)
    return flowcases.tcp_segment(f["src"], f["dst"], f["sport"], f["dport"], flowcases.SYN, bytes([salt]) * (salt % 3))


def fillers():
    return [flowcases.tcp_segment((10, 0, 0, 1), (10, 0, 0, 2), 1000, 2000, flowcases.SYN),
            flowcases.eth_ip4((1, 1, 1, 1), (2, 2, 2, 2), 0xcc, 1, 0, 28, payload=b"x" * 8)]


def c6_packets(seed, n):
    data, off, cap = synth.host_batch(6, seed, n)
    return [bytes(data[o:o + c]) for o, c in zip(off, cap)]


def test_restatement_holds(gpu_ctx):
    """Grouper.hashes of every keyed IPv4 and IPv6 packet, from gpk_group_batch
    (key_kernel) and from gpk_decode_group_batch (the fused derive_key), is
    grouphash's value for the oracle's key."""
    pk = pktutil.fuzz_packets(17, 2500) + flowcases.connection_cases() + list(flowcases.defrag_frames()[0].values())
    pk += [f for _, f in flowcases.defrag_struct_cases()] + c6_packets(5, 1000)
    P = Decoded(gpu_ctx, pk)
    g = flows.Grouper(len(pk))
    for name, kind in KIND.items():
        _, codes, _ = P.oracle(kind)
        idx = [i for i, c in enumerate(codes) if c >= 0]
        keys = [FO.packet_key(kind, pk[i], P.ref["records"][i], P.ref["layouts"][i], 0, 8) for i in idx]
        assert len(idx) > 100 and any(k[1][0] == 1 for k in keys), (name, len(idx))
        want = H.hash_words(np.array([H.key_words(k) for k in keys], np.uint32))
        for entry, run in (("group", check_group), ("decode_group", check_fused)):
            run(g, P, kind)
            got = g.hashes(len(pk))[idx]
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, ("tests/grouphash.py no longer restates the device's key words or hash: update it",
                                   name, entry, len(bad), len(idx), keys[bad[0]], hex(int(got[bad[0]])),
                                   hex(int(want[bad[0]])))
    with pytest.raises(Exception):
        g.hashes(len(pk) + 1)
    g.close()


@pytest.mark.parametrize("name", ["frag", "conn"])
def test_equal_tag_different_key(gpu_ctx, name):
    """Two different keys whose hashes share tag and home slot in the 16-slot
    table of a Grouper(8), interleaved: the tag comparison cannot tell them
    apart, only the key words do. Both orders, both entry points."""
    pairs, stats = H.find_pairs(name, H.table_size(8))
    assert len(pairs) >= 2, stats
    kind = KIND[name]
    g = flows.Grouper(8)
    for a, b in pairs[:4]:
        for x, y in ((a, b), (b, a)):
            pk = [packet_of(name, c, k) for k, c in enumerate((x, y, x, y, x, y))] + fillers()
            P = Decoded(gpu_ctx, pk)
            for run in (check_group, check_fused):
                run(g, P, kind, what=(a, b, stats))
                h = [int(v) for v in g.hashes(2)]
                assert h[0] != h[1] and h[0] >> 28 == h[1] >> 28 and (h[0] ^ h[1]) & 15 == 0, (a, b, h, stats)
            groups, codes, _ = P.oracle(kind)
            assert codes[:6] == [0, 1, 0, 1, 0, 1], (codes, stats)  # the case is what it claims to be
    g.close()


@pytest.mark.parametrize("name", ["frag", "conn"])
@pytest.mark.parametrize("slots", [(1020, 1021, 1022, 1023), (1023,)])
def test_long_wrapping_chains(gpu_ctx, name, slots):
    """300 distinct keys homed on the last 4 slots (or all on the last slot) of
    the 1024-slot table of a Grouper(512): probe chains of 75 to 300 keys that
    wrap to slot 0. 150 keys come once, 100 twice, 50 three times (500 packets:
    the grouper holds 512), shuffled."""
    T = H.table_size(512)
    assert T == 1024
    cands, stats = H.find_homed(name, T, slots, 300)
    assert len(cands) >= 300, stats
    rng = np.random.default_rng(21)
    reps = np.repeat(np.arange(300), np.repeat([1, 2, 3], [150, 100, 50])[rng.permutation(300)])
    order = reps[rng.permutation(len(reps))]
    assert len(order) == 500
    pk = [packet_of(name, cands[k], j & 255) for j, k in enumerate(order)]
    P = Decoded(gpu_ctx, pk)
    g = flows.Grouper(512)
    for run in (check_group, check_fused):
        out = run(g, P, KIND[name], what=stats)
        assert int(out["counts"][0]) == 300, stats
        home = g.hashes(len(pk)) & np.uint64(T - 1)
        assert set(home.tolist()) == set(slots), stats  # the case is what it claims to be
    g.close()


@pytest.mark.parametrize("name", ["frag", "conn"])
@pytest.mark.parametrize("nkeys", [3, 1])
def test_elephants_and_first_index_races(gpu_ctx, name, nkeys):
    """60 000 packets of three keys that first appear at packets 0, 1 and
    59 999 (the rest are the first two, pseudo-randomly), and of one key: every
    packet of a key meets the others on one slot word, whose index field must
    end as the smallest. The groups here come from numpy on the known key
    labels (which packet was built from which key), not from the oracle."""
    n = 60000
    rng = np.random.default_rng(8)
    lab = rng.integers(0, 2, n) if nkeys == 3 else np.zeros(n, np.int64)
    if nkeys == 3:
        lab[0], lab[1], lab[n - 1] = 0, 1, 2
    three = [packet_of(name, c) for c in (11, 70001, 140001)]
    pk = [three[k] for k in lab]
    groups = [np.nonzero(lab == k)[0].tolist() for k in range(nkeys)]
    data, off, cap = pktutil.pack(pk)
    import torch
    d = torch.from_numpy(data).cuda()
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    c = torch.from_numpy(cap.astype(np.int32)).cuda()
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    parser = flowcases_parser()
    gpu_ctx.decode_device(parser, d, o, c, rec, None, fl, lay, stream=torch.cuda.current_stream())
    g = flows.Grouper(n)
    out = g.group(d, o, c, rec, lay, fl, kind=KIND[name], out=poisoned(n))
    torch.cuda.synchronize()
    compare(out, groups, lab.tolist(), ("group", name, nkeys))
    rec2 = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    out = g.decode_group(gpu_ctx, parser, d, o, c, rec2, None, fl, kind=KIND[name], out=poisoned(n))
    torch.cuda.synchronize()
    compare(out, groups, lab.tolist(), ("decode_group", name, nkeys))
    assert torch.equal(rec2, rec)
    g.close()


def flowcases_parser():
    from configs import device_parser
    return device_parser(flowcases.DEFRAG_PARSER)


@pytest.fixture(scope="module")
def bucket_batches(gpu_ctx):
    cache = {}

    def get(n):
        if n not in cache:
            none = [b"\x00" * 10, flowcases.MAC + b"\x08\x06" + b"\x00" * 28, b""]
            cache[n] = Decoded(gpu_ctx, none + c6_packets(9, n) + none)
        return cache[n]
    return get


@pytest.mark.parametrize("buckets,n", [(1, 5000), (2, 5000), (4096, 5000), (8192, 5000), (65536, 5000),
                                       (8192, 12000)])
def test_buckets(gpu_ctx, bucket_batches, buckets, n):
    """NET_BUCKET on both sides of the 4096-bucket branch (the buckets' ranks
    as the sort key up to 4096 buckets; above, the buckets' first packets with
    the batch size as the sentinel), and at 1 and 65536 buckets: C6 packets
    between packets without a network layer. Both branches sort by first
    appearance, so which of them runs changes the cost and not the result;
    what is pinned is that each gives the oracle's groups. 12 000 packets in
    8192 buckets have first packets past index 8192: a sentinel taken from
    the bucket count there would lose them."""
    P = bucket_batches(n)
    g = flows.Grouper(P.n)
    out = check_group(g, P, FO.NET_BUCKET, buckets)
    G = int(out["counts"][0])
    assert G == 1 if buckets == 1 else G > 1, (buckets, G)
    if n > buckets:
        assert max(grp[0] for grp in P.oracle(FO.NET_BUCKET, buckets)[0]) > buckets
    g.close()
