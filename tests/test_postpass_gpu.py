"""The two passes of csrc/gpk_postpass.h, gpk_tunnel_batch and
gpk_control_batch, run the same kernels and own the same carved workspace.
Each case runs for both: the device against the pass's own host twin
(peel_host / decode_host) on the same batch and the same decode, every output
array whole and the entries below counts[0] field by field, outputs pre-filled
so that nothing written past the list goes unseen. The compaction at its wave
and block boundaries, handles of the smallest workspace and of a full one used
twice, the stream and the device, and what create refuses. No tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import configs
import controlcases as CC
import tunnelcases as TC
from gopacket_amd import _lib, flows
from pktutil import pack

pytestmark = pytest.mark.gpu
FILL = 0xA5


class Pass:
    def __init__(self, cls, device, host, cfg, cases, names, create, limit):
        self.cls, self.cfg, self.create, self.limit = cls, cfg, create, limit
        self.device, self.host = device, getattr(cls, host)
        c = dict(cases)
        self.cand, self.plain = [c[k] for k in names], c["plain_tcp"]  # the candidates interleave every class

    def batch(self, n, where):
        """n packets; those whose index is in `where` are candidates, the classes taking turns."""
        return [self.cand[i % len(self.cand)] if i in where else self.plain for i in range(n)]


PASSES = dict(
    tunnel=Pass(flows.Detunneler, "peel", "peel_host", TC.PARSER, TC.quirk_cases()[0],
                ("gre_plain", "vxlan_plain", "geneve_len6", "gre_checksum_good", "geneve_dot1q", "gre_ipv6",
                 "gre_checksum_bad", "geneve_unregistered"), "gpk_tunneler_create", 1 << 32),
    control=Pass(flows.ControlDecoder, "decode", "decode_host", CC.PARSER, CC.quirk_cases()[0],
                 ("icmp6_echo_request", "arp_len7", "icmp4_echo", "arp_reply_padded_60", "icmp4_bad_checksum"),
                 "gpk_controller_create", 1 << 28))


@pytest.fixture(params=sorted(PASSES))
def pas(request):
    return PASSES[request.param]


def dev(a):
    a = np.array(a)  # a writable copy
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}.get(a.dtype.itemsize, a.dtype))).cuda()


def run(ctx, pas, packets, handle=None, stream=None):
    """Decode on the device, run the pass there and its host twin on the same
    records and layouts, compare, and return the device's outputs as host arrays."""
    data, offs, caps = pack(packets)
    n = len(caps)
    p = configs.device_parser(pas.cfg)
    d = dev(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)]))
    o, c = dev(offs), dev(caps)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    ctx.decode_device(p, d, o, c, rec, err, fl, lay)
    shape = {key: (count(n), np.dtype(dt)) for key, count, dt in pas.cls.OUTPUTS}
    out = {key: torch.full((k * dt.itemsize,), FILL, dtype=torch.uint8, device="cuda")
           for key, (k, dt) in shape.items()}
    h = handle or pas.cls(max(n, 1))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    getattr(h, pas.device)(ctx, d, o, c, rec, lay, p, out=out, stream=stream)
    torch.cuda.synchronize()
    if handle is None:
        h.close()
    got = {key: out[key].cpu().numpy().view(shape[key][1]) for key in out}
    want = pas.host(data, offs, caps, rec.cpu().numpy().view(_lib.RECORD_DTYPE),
                    lay.cpu().numpy().view(_lib.LAYOUT_DTYPE), p, fill=FILL)
    m = int(want["counts"][0])
    assert set(got) == set(want) == set(pas.cls.KEYS)
    for key in pas.cls.KEYS:  # whole arrays: what the twin leaves at the fill byte the device must not touch
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
        per_packet = len(want[key]) == n and key != "verdict"
        for f in want[key].dtype.names or ():
            assert np.array_equal(got[key][:m][f], want[key][:m][f]), (key, f)
        if per_packet:
            assert np.all(got[key][m:].view(np.uint8) == FILL), key
    return got


def ordered(pas, got):
    """The list is ordered by class and, inside a class, by packet index."""
    cs = got["class_start"].astype(np.int64)
    for c in range(len(cs) - 1):
        assert np.all(np.diff(got["index"][cs[c]:cs[c + 1]].astype(np.int64)) > 0)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257])
def test_candidate_count_among_plain_packets(gpu_ctx, pas, m):
    """Exactly m candidates among 257 packets (a full block and one packet)."""
    where = set(np.random.RandomState(m).choice(257, m, replace=False).tolist())
    got = run(gpu_ctx, pas, pas.batch(257, where))
    assert int(got["counts"][0]) == m and int((got["verdict"] >= 0).sum()) == m
    assert m < len(pas.cand) or int(got["counts"][len(got["class_start"])]) > 0  # sums were made
    ordered(pas, got)


def test_candidates_only_in_the_last_block(gpu_ctx, pas):
    got = run(gpu_ctx, pas, pas.batch(257, {256}))
    assert int(got["counts"][0]) == 1 and int(got["index"][0]) == 256 and int(got["verdict"][256]) == 0
    assert np.all(got["verdict"][:256] == -1)


def test_255_packets(gpu_ctx, pas):
    """One packet short of a block, every packet and every other packet a candidate."""
    for where in (set(range(255)), set(range(0, 255, 2))):
        got = run(gpu_ctx, pas, pas.batch(255, where))
        assert int(got["counts"][0]) == len(where)
        ordered(pas, got)


def test_handle_of_one_packet(gpu_ctx, pas):
    """The smallest workspace: every array borders its neighbour inside a 256-byte granule."""
    h = pas.cls(1)
    for pk in (pas.cand[0], pas.plain, pas.cand[2]):
        got = run(gpu_ctx, pas, [pk], handle=h)
        assert int(got["counts"][0]) == (pk is not pas.plain)
    h.close()


def test_full_handle_twice(gpu_ctx, pas):
    """max_packets = n = 65, one more than a wave, then a different batch with another
    class mix on the workspace the first call used."""
    h = pas.cls(65)
    first = run(gpu_ctx, pas, pas.batch(65, set(range(65))), handle=h)
    second = run(gpu_ctx, pas, [pas.plain if i % 3 == 0 else pas.cand[(i // 3) % 2] for i in range(65)], handle=h)
    assert int(first["counts"][0]) == 65 and int(second["counts"][0]) == 43
    assert first["counts"].tolist() != second["counts"].tolist()
    assert first["class_start"].tolist() != second["class_start"].tolist()
    with pytest.raises(_lib.GpkError):
        run(gpu_ctx, pas, [pas.plain] * 66, handle=h)
    h.close()


def test_stream_and_device_are_left_alone(gpu_ctx, pas):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    before = torch.cuda.current_device()
    h = pas.cls(100, before)
    got = run(gpu_ctx, pas, pas.batch(100, set(range(0, 100, 3))), handle=h, stream=torch.cuda.Stream())
    assert torch.cuda.current_device() == before and int(got["counts"][0]) == 34
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = pas.cls(16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    h.close()
    assert torch.cuda.current_device() == before


def test_create_refusals(gpu_ctx, pas):
    create = getattr(_lib.lib(), pas.create)
    destroy = getattr(_lib.lib(), pas.create.replace("create", "destroy"))
    for cap in (0, pas.limit):
        h = ctypes.c_void_p()
        assert create(ctypes.byref(h), 0, cap) == _lib.GPK_EINVAL and not h
        with pytest.raises(_lib.GpkError, match=r"\(%d\)" % _lib.GPK_EINVAL):
            pas.cls(cap)
    assert create(None, 0, 8) == _lib.GPK_EINVAL
    for device in (torch.cuda.device_count(), -1):
        h = ctypes.c_void_p()
        assert create(ctypes.byref(h), device, 8) == _lib.GPK_ENODEV and not h
    h = ctypes.c_void_p()  # the refusals left nothing behind that stops a good create
    assert create(ctypes.byref(h), 0, 8) == _lib.GPK_OK and h
    assert destroy(h) == _lib.GPK_OK


def test_tunneler_accepts_what_the_controller_refuses(gpu_ctx):
    """gpk_tunnel.h documents max_packets < 2^32, gpk_control.h < 2^28. The tunneler's
    workspace for 2^28 packets is about 60 MB: made and released, nothing runs on it."""
    h = ctypes.c_void_p()
    assert _lib.lib().gpk_tunneler_create(ctypes.byref(h), 0, 1 << 28) == _lib.GPK_OK and h
    assert _lib.lib().gpk_tunneler_destroy(h) == _lib.GPK_OK
