"""The pipeline handles on one carved workspace (csrc/gpk_workspace.h): a handle
of one packet, where every array borders its neighbour inside a 256-byte
granule; a handle filled exactly, one packet past a wave, and used again for a
different batch, so that nothing a call leaves in the workspace reaches the
next; and what gpk_*_create refuses. Every result is compared with the
pipeline's model by its own suite's check (test_flows_gpu's flowcheck,
test_defrag_gpu, test_defrag6_gpu, test_tcpasm_gpu). No tolerance anywhere."""
import ctypes

import pytest

import defrag6cases as DC6
import defragcases as DC4
import tcpasmcases as TC
import test_defrag6_gpu as T6
import test_defrag_gpu as T4
import test_tcpasm_gpu as TT
from flowcheck import DEFRAG6, Decoded, check_fused, check_group
from gopacket_amd import _lib, flows
from oracle import flows_oracle as FO

pytestmark = pytest.mark.gpu

FULL = 65  # one more than a wave: both plan instantiations' grids and a partial last block
HANDLES = ("Grouper", "Defragmenter", "Defragmenter6", "Assembler")


class Keeper:
    """Stands in for a handle class of gopacket_amd.flows: hands out one handle,
    whose close() leaves it open, however often it is asked."""

    def __init__(self, name, cls, made):
        self.name, self.cls, self.made, self.handle = name, cls, made, None

    def __call__(self, max_packets, device=0):
        if self.handle is None:
            h = self.handle = self.cls(max_packets, device)
            h.really_close, h.close = h.close, lambda: None
            self.made[self.name] = h
        assert self.handle.max_packets == max_packets, "a kept handle serves one size"
        return self.handle

    def __getattr__(self, name):  # the class's static helpers (Grouper.to_lists)
        return getattr(self.cls, name)


@pytest.fixture
def kept(monkeypatch):
    """The suites' checks make their handles with flows.<Class>(len(packets))
    and close them. Inside this fixture each class hands out one handle for the
    whole test: a second check of as many packets runs on the workspace the
    first one used. Yields {class name: handle} of the handles made so far."""
    made = {}
    keepers = [Keeper(name, getattr(flows, name), made) for name in HANDLES]
    for k in keepers:
        monkeypatch.setattr(flows, k.name, k)
    yield made
    for h in made.values():
        h.really_close()


def test_kept_handles_are_kept(gpu_ctx, kept):
    """The fixture does what the tests below rely on."""
    a = flows.Defragmenter(3)
    a.close()
    assert flows.Defragmenter(3) is a and a.h and kept == {"Defragmenter": a}


# ---- a handle at the smallest workspace: max_packets = n = 1
def test_one_packet_grouper(gpu_ctx):
    g = flows.Grouper(1)
    for pk, kinds in ((TC.seg(1000, TC.SYN), (FO.CONNECTION, FO.NET_BUCKET)),
                      (DC4.frag(7, 0, 1, bytes(range(24))), (FO.DEFRAG, FO.NET_BUCKET)),
                      (DC6.frag6(7, 0, 1, bytes(range(24))), (DEFRAG6,))):
        P = Decoded(gpu_ctx, [pk])
        for kind in kinds:
            out = check_group(g, P, kind, what="one packet")
            assert out["counts"].cpu().tolist() == [1, 1]  # keyed: the table, the sort and the scan all ran
            if kind in (FO.CONNECTION, FO.DEFRAG):
                check_fused(g, P, kind, what="one packet")
    g.close()


def test_one_packet_defragmenters(gpu_ctx):
    ref, got, _ = T4.check(gpu_ctx, [DC4.frag(7, 0, 1, bytes(range(24)))])  # a lone first fragment
    assert got["verdict"] == [T4.M.HELD] and got["pending"] == [0]
    ref, got, _ = T6.check(gpu_ctx, [DC6.frag6(7, 0, 1, bytes(range(24)))])
    assert got["verdict"] == [T6.H] and got["pending"] == [0]


def test_one_packet_assembler(gpu_ctx):
    ref, got = TT.check(gpu_ctx, [TC.seg(1000, TC.SYN)])  # a lone SYN: a stream, and an open connection
    assert got["verdict"] == [TT.M.DIRECT] and got["counts"][0] == 1 and got["counts"][4] == 1
    ref, got = TT.check(gpu_ctx, [TC.seg(1000, TC.SYN)], flush=True)
    assert got["counts"][4] == 0


# ---- a handle filled exactly, then used again: max_packets = n = 65, two different batches
def two_batches(packets):
    assert len(packets) >= 2 * FULL
    return packets[:FULL], packets[FULL:2 * FULL]


def test_full_grouper_twice(gpu_ctx):
    tcp = two_batches(TC.random_traffic(11, 40))
    f4 = two_batches(DC4.random_traffic(12, 40, lo=200, hi=900, per=104, window=6))
    f6 = two_batches(DC6.random_traffic(13, 40, lo=200, hi=900, per=104, window=6))
    g = flows.Grouper(FULL)
    for k in (0, 1):
        mixed = (tcp[k][:22] + f4[k][:22] + f6[k][:21])  # every kind has keyed and unkeyed packets
        assert len(mixed) == FULL
        P = Decoded(gpu_ctx, mixed)
        for kind in (FO.CONNECTION, FO.DEFRAG, FO.NET_BUCKET, DEFRAG6):
            out = check_group(g, P, kind, what=("full", k))
            G, K = out["counts"].cpu().tolist()
            assert 1 < G and (K < FULL or kind == FO.NET_BUCKET)  # a bucket for every packet with a network layer
        for kind in (FO.CONNECTION, FO.DEFRAG):
            check_fused(g, P, kind, what=("full", k))
    g.close()


def test_full_defragmenter_twice(gpu_ctx, kept):
    for k, pk in enumerate(two_batches(DC4.random_traffic(12, 40, lo=200, hi=900, per=104, window=6))):
        ref, got, _ = T4.check(gpu_ctx, pk)
        assert ref["datagrams"] and T4.M.HELD in ref["verdict"] and ref["pending"], k
    assert set(kept) == {"Grouper", "Defragmenter"}


def test_full_defragmenter6_twice(gpu_ctx, kept):
    for k, pk in enumerate(two_batches(DC6.random_traffic(13, 40, lo=200, hi=900, per=104, window=6))):
        ref, got, _ = T6.check(gpu_ctx, pk)
        assert ref["datagrams"] and T6.H in ref["verdict"] and ref["pending"], k
    assert set(kept) == {"Grouper", "Defragmenter6"}


@pytest.mark.parametrize("max_pages,flush", [(0, False), (4, True)])
def test_full_assembler_twice(gpu_ctx, kept, max_pages, flush):
    for k, pk in enumerate(two_batches(TC.random_traffic(11, 40))):
        ref, got = TT.check(gpu_ctx, pk, max_pages=max_pages, flush=flush)
        assert ref["counts"][0] > 1 and ref["counts"][1] > 1, k  # streams, chunks
    assert set(kept) == {"Grouper", "Assembler"}


# ---- what create refuses (gpk_grouper_create: test_flows_gpu.test_einval_contract)
@pytest.mark.parametrize("entry,cls", [("gpk_defragger_create", "Defragmenter"),
                                       ("gpk_defragger6_create", "Defragmenter6"),
                                       ("gpk_tcpasm_create", "Assembler")])
def test_create_refusals(gpu_ctx, entry, cls):
    import torch
    create = getattr(_lib.lib(), entry)
    for cap in (0, 1 << 28):
        h = ctypes.c_void_p()
        assert create(ctypes.byref(h), 0, cap) == _lib.GPK_EINVAL and not h
        with pytest.raises(_lib.GpkError, match=r"\(%d\)" % _lib.GPK_EINVAL):
            getattr(flows, cls)(cap)
    assert create(None, 0, 8) == _lib.GPK_EINVAL
    for device in (torch.cuda.device_count(), -1):
        h = ctypes.c_void_p()
        assert create(ctypes.byref(h), device, 8) == _lib.GPK_ENODEV and not h
    h = ctypes.c_void_p()  # the refusals left nothing behind that stops a good create
    assert create(ctypes.byref(h), 0, 8) == _lib.GPK_OK and h
    assert getattr(_lib.lib(), entry.replace("create", "destroy"))(h) == _lib.GPK_OK
