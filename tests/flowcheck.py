"""Shared by the grouping tests: a batch decoded on the device and by the
decode oracle, and the comparison of gpk_group_batch / gpk_decode_group_batch
with oracle/flows_oracle.py on it (what test_flows_gpu.check does, in pieces,
for batches in any layout and groupers that outlive a call)."""
import numpy as np

import flowcases
import pktutil
from configs import device_parser, oracle_parser
from oracle import flows_oracle as FO

POISON = 0x5A5A5A5A
DEFRAG6 = 4  # GPK_GROUP_DEFRAG6: its reference is tests/defrag6_model.py, not flows_oracle


class Decoded:
    """packets: list of bytes, in batch order. batch: (data, offsets, caplens)
    numpy arrays that hold them (default: packed), or device tensors with
    `device_batch`. The oracle always decodes the packed packets; `share`
    is a Decoded of the same packets whose oracle results are taken over."""

    def __init__(self, gpu_ctx, packets, cfg=flowcases.DEFRAG_PARSER, batch=None, device_batch=None, share=None):
        import torch
        self.ctx, self.cfg, self.packets, self.n = gpu_ctx, cfg, packets, len(packets)
        pd, po, pc = pktutil.pack(packets)
        self.ref = share.ref if share is not None else oracle_parser(cfg).decode(pd, po, pc, layouts=True)
        if device_batch is not None:
            self.d, self.o, self.c = device_batch
        else:
            data, off, cap = batch if batch is not None else (pd, po, pc)
            self.d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
            self.o = torch.from_numpy(off.astype(np.int64)).cuda()
            self.c = torch.from_numpy(cap.astype(np.int32)).cuda()
        n = max(self.n, 1)
        self.rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        self.err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
        self.fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
        self.lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        self.parser = device_parser(cfg)
        gpu_ctx.decode_device(self.parser, self.d, self.o, self.c, self.rec, self.err, self.fl, self.lay,
                              stream=torch.cuda.current_stream())
        self._oracle = share._oracle if share is not None else {}

    def oracle(self, kind, buckets=8):
        """(groups: list of index lists in first-appearance order, codes) of the oracle, cached."""
        key = (kind, buckets if kind == FO.NET_BUCKET else 0)
        if key not in self._oracle:
            if kind == DEFRAG6:  # the keying rule of the IPv6 reassembly model
                import defrag6_model
                og, oc = defrag6_model.group(self.packets, self.ref["layouts"])
            else:
                og, oc = FO.group(kind, self.packets, self.ref["records"], self.ref["layouts"], self.ref["flows"],
                                  buckets)
            self._oracle[key] = (list(og.values()), oc, list(og.keys()))
        return self._oracle[key]


def poisoned(n):
    """Output tensors of a grouping call, every element POISON."""
    import torch
    return dict(group_of=torch.full((n,), POISON, dtype=torch.int32, device="cuda"),
                perm=torch.full((n,), POISON, dtype=torch.int32, device="cuda"),
                start=torch.full((n + 1,), POISON, dtype=torch.int32, device="cuda"),
                first=torch.full((max(n, 1),), POISON, dtype=torch.int32, device="cuda"),
                counts=torch.full((2,), POISON, dtype=torch.int32, device="cuda"))


def compare(out, groups, codes, what):
    """The device's result `out` is exactly the oracle's (groups, codes): counts,
    group_of, start[:G+1], first[:G], perm[:K], and perm[K:] a permutation of
    the unkeyed packets ("keyed packets first")."""
    n = len(codes)
    G, K = out["counts"].cpu().tolist()
    assert (G, K) == (len(groups), sum(len(g) for g in groups)), (what, G, K, len(groups))
    gof = out["group_of"].cpu().tolist()
    assert gof == codes, (what, [(i, a, b) for i, (a, b) in enumerate(zip(gof, codes)) if a != b][:5])
    perm = out["perm"].cpu().tolist()
    start = out["start"][:G + 1].cpu().tolist()
    assert start == list(np.concatenate([[0], np.cumsum([len(g) for g in groups], dtype=np.int64)])), what
    got = [perm[start[g]:start[g + 1]] for g in range(G)]
    assert got == groups, (what, [(g, a[:5], b[:5]) for g, (a, b) in enumerate(zip(got, groups)) if a != b][:3])
    assert out["first"][:G].cpu().tolist() == [g[0] for g in groups], what
    assert sorted(perm[K:]) == [i for i in range(n) if codes[i] < 0], what


def check_group(g, P, kind, buckets=8, what=""):
    """gpk_group_batch of the decoded batch P on grouper g against the oracle."""
    import torch
    out = g.group(P.d, P.o, P.c, P.rec, P.lay, P.fl, kind=kind, buckets=buckets, out=poisoned(P.n))
    torch.cuda.synchronize()
    groups, codes, _ = P.oracle(kind, buckets)
    compare(out, groups, codes, ("group", kind, buckets, what))
    return out


def check_fused(g, P, kind, what=""):
    """gpk_decode_group_batch against the oracle, and its records and flows
    against the plain decode of the same batch."""
    import torch
    n = max(P.n, 1)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    out = g.decode_group(P.ctx, P.parser, P.d, P.o, P.c, rec, err, fl, kind=kind, out=poisoned(P.n))
    torch.cuda.synchronize()
    groups, codes, _ = P.oracle(kind)
    compare(out, groups, codes, ("decode_group", kind, what))
    assert torch.equal(rec, P.rec) and torch.equal(fl, P.fl), ("decode_group records/flows", kind, what)
    return out
