"""TLS over reassembled streams on the device (include/gpk_tls_streams.h):
flows.TLSStreams (TCPAssembler, then gpk_tls_streams) against the model
(tlsstream_model.py) field for field, and gpk_tls_streams against its host twin
byte for byte on the device's own reassembly, for every case of
tlsstreamcases.py: every split position in one call and in two, the largest
record, TCP order and overlap, loss, close, no SYN, bytes that are no TLS, the
server direction, block and wave edges, the port table; a seeded mix in three
calls; the capacity retry; handle reuse, stream and device."""
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

import configs
import tls_model as M
import tlscases as C
import tlsstream_model as SM
import tlsstreamcases as SC
from gopacket_amd import _lib, flows
from pktutil import pack
from tlsstreamutil import assert_same_streams, names_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in SC.cases()}
SPARE = (3, 2, 5, 7)


def upload(packets):
    data, offs, caps = pack(packets)
    d = torch.from_numpy(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)])).cuda()
    return d, torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(caps.astype(np.int32)).cuda()


def host_arrays(ts):
    """The arrays the last gpk_tls_streams call of `ts` worked on, on the host."""
    last = ts.asm._last
    o = last["out"]
    asm = {k: o[k].cpu().numpy() for k in ("stream_first", "stream_closed", "stream_data0", "counts", "data")}
    asm["chunks"] = o["chunks"].cpu().numpy().view(_lib.TCP_CHUNK_DTYPE)
    carry = ts._last_call["carry"]
    carry = tuple(None if t is None else t.cpu().numpy() for t in carry)
    n = last["offsets"].numel()
    return (last["data"].cpu().numpy(), last["offsets"].cpu().numpy(), last["caplens"].cpu().numpy(),
            last["records"].cpu().numpy().view(_lib.RECORD_DTYPE)[:n],
            last["layouts"].cpu().numpy().view(_lib.LAYOUT_DTYPE)[:n], asm, carry)


def device_again(ts, caps, fill=0xA5, stream=None, decoder=None):
    """The last call of `ts` once more on the device, into arenas of `caps`
    that start as `fill` bytes; -> host arrays."""
    last = ts.asm._last
    n = last["offsets"].numel()
    out = dict(streams=torch.full((max(n, 1) * 64,), fill, dtype=torch.uint8, device="cuda"),
               recs=torch.full((caps[0] * 32,), fill, dtype=torch.uint8, device="cuda"),
               hellos=torch.full((caps[1] * 64,), fill, dtype=torch.uint8, device="cuda"),
               snis=torch.full((caps[2],), fill, dtype=torch.uint8, device="cuda"),
               tails=torch.full((caps[3],), fill, dtype=torch.uint8, device="cuda"),
               counts=torch.full((12,), -1, dtype=torch.int64, device="cuda"))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    (decoder or ts.decoder).decode(ts.ctx, ts.parser, last["data"], last["offsets"], last["caplens"], last["records"],
                                   last["layouts"], last["out"], *caps, carry=ts._last_call["carry"],
                                   frame_unstarted=ts.frame_unstarted, out=out, stream=stream)
    torch.cuda.synchronize()
    return dict(streams=out["streams"].cpu().numpy().view(_lib.TLS_STREAM_DTYPE),
                recs=out["recs"].cpu().numpy().view(_lib.TLS_STREAM_REC_DTYPE),
                hellos=out["hellos"].cpu().numpy().view(_lib.TLS_HELLO_DTYPE), snis=out["snis"].cpu().numpy(),
                tails=out["tails"].cpu().numpy(), counts=out["counts"].cpu().numpy().view(np.uint64))


def host_twin(ts, caps, fill=0xA5):
    data, offs, cl, rec, lay, asm, carry = host_arrays(ts)
    return flows.TLSStreamDecoder.decode_host(ts.parser, data, offs, cl, rec, lay, asm, *caps, carry=carry,
                                              frame_unstarted=ts.frame_unstarted, fill=fill)


def check_call(ts, res, want, what):
    """One call: the wrapper's result against the model field for field, and
    the device against the host twin byte for byte, the arenas SPARE longer
    than needed (the device must leave those bytes alone)."""
    assert len(res.streams) == len(want), (what, len(res.streams), len(want))
    if not want:
        return
    for j, (s, d) in enumerate(zip(res.streams, want)):
        assert (s["id"], s["state"], s["tail_in"]) == (d["id"], d["state"], d["tail_in"]), (what, j, s, d)
        rows = SM.to_arrays([dict(d, framed=True)], 1)
        rows["recs"]["stream"] = j
        assert s["recs"].tobytes() == rows["recs"].tobytes(), (what, j, s["recs"], rows["recs"])
        assert s["names"] == [e["client_hello"]["sni"] if e["client_hello"]["has_sni"] else None
                              for e in d["entries"] if "client_hello" in e], (what, j)
        assert len(s["hellos"]) == len(s["names"]) and (s["closed"] is not None) == d["closed"]
    assert res.snis() == names_of(want)
    need = flows.TLSStreamDecoder.needed(res.counts)
    caps = tuple(a + b for a, b in zip(need, SPARE))
    dv, h = device_again(ts, caps), host_twin(ts, caps)
    assert_same_streams(h, dv, what)
    assert not int(dv["counts"][5]) and int(dv["counts"][0]) == len(want)
    # the tails the model keeps are the bytes in the arena
    for e, d in zip(dv["streams"], want):
        a = int(e["tail_off"])
        assert bytes(dv["tails"][a:a + int(e["tail_len"])]) == bytes(d["tail"]), what


def run_case(ctx, case, cfg=SC.PARSER, max_packets=None):
    model = SM.Streaming(cfg, case["max_pages"], case["frame_unstarted"])
    n = max(len(pk) for pk in case["calls"])
    ts = flows.TLSStreams(ctx, configs.device_parser(cfg), max_packets or n + 64, max_pages=case["max_pages"],
                          frame_unstarted=case["frame_unstarted"])
    calls = []
    for k, pk in enumerate(case["calls"]):
        want = model.feed(pk)
        res = ts.feed(*upload(pk))
        check_call(ts, res, want, "%s call %d" % (case["name"], k))
        calls.append((res, want))
    if case["flush"]:
        want = model.flush_all()
        res = ts.flush_all()
        check_call(ts, res, want, "%s flush" % case["name"])
        calls.append((res, want))
    ts.close()
    return calls


@pytest.mark.parametrize("name", list(CASES))
def test_case(gpu_ctx, name):
    run_case(gpu_ctx, CASES[name])


@pytest.mark.parametrize("two", [False, True], ids=["one_call", "two_calls"])
def test_every_split_position(gpu_ctx, two):
    """One stream per cut position: every stream yields the same records and
    the server name; the same packets through gpk_tls_batch give "TLS packet
    length mismatch" wherever the cut is inside a record."""
    calls = run_case(gpu_ctx, CASES["split_two_calls" if two else "split_one_call"])
    n = len(SC.flight()) - 1
    got = {}
    for res, _ in calls:
        for s in res.streams:
            got.setdefault(s["id"], []).extend((int(r["rec"]["content_type"]), int(r["rec"]["length"]), int(r["err"]))
                                               for r in s["recs"])
    H = len(SC.hello_rec())
    assert all(got[g] == [(22, H - 5, 0), (20, 1, 0), (23, 40, 0)] for g in range(n))
    assert sorted(x for res, _ in calls for x in res.snis()) == [(g, b"split.example") for g in range(n)]
    if two:
        assert [s["tail_in"] for s in calls[1][0].streams][:4] == [1, 2, 3, 4]  # a seam inside the header
        return
    pk = [p for p in CASES["split_one_call"]["calls"][0] if len(p) > 54]
    d, o, c = upload(pk)
    p = configs.device_parser(C.PARSER)
    m = len(pk)
    rec = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
    lay = torch.zeros(m * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(p, d, o, c, rec, torch.zeros(2 * m, dtype=torch.int32, device="cuda"),
                          torch.zeros(3 * m, dtype=torch.int64, device="cuda"), lay)
    tld = flows.TLSDecoder(m)
    out = tld.decode_all(gpu_ctx, d, o, c, rec, lay, p)
    torch.cuda.synchronize()
    recs = out["records"].cpu().numpy().view(_lib.TLS_DTYPE)
    verdict = out["verdict"].cpu().numpy()
    first = [int(recs[int(verdict[i])]["err"]) for i in range(0, m, 2)]
    assert first[4:H - 1] == [M.E_LEN] * (H - 5) and first[:4] == [M.E_REC_SHORT] * 4
    hel = out["hellos"].cpu().numpy().view(_lib.TLS_HELLO_DTYPE)
    assert sorted(int(h["packet"]) for h in hel if int(h["has_sni"])) == [2 * (H - 1), 2 * (H + 6 - 1)]
    tld.close()


def test_largest_record_tail(gpu_ctx):
    calls = run_case(gpu_ctx, CASES["largest_record"])
    assert [len(w[0]["tail"]) for _, w in calls] == [20 * SC.MSS, _lib.TLSS_MAX_TAIL, 0]
    assert [(int(r["rec"]["content_type"]), int(r["rec"]["length"])) for r in calls[2][0].streams[0]["recs"]] == [
        (23, 65535), (21, 2)]
    assert calls[2][0].streams[0]["tail_in"] == 65539


def test_sticky_states(gpu_ctx):
    (a, _), (b, _) = run_case(gpu_ctx, CASES["not_tls_is_sticky"])
    assert [int(r["err"]) for r in a.streams[0]["recs"]] == [0, 0, M.E_REC_TYPE] and a.streams[0]["state"] == SM.NOT_TLS
    assert b.streams[0]["state"] == SM.NOT_TLS and len(b.streams[0]["recs"]) == 0
    (a, _), (b, _) = run_case(gpu_ctx, CASES["page_limit_forces_a_skip"])
    assert a.streams[0]["state"] == b.streams[0]["state"] == SM.LOST and len(b.streams[0]["recs"]) == 0
    assert int(a.streams[0]["recs"][-1]["err"]) == M.E_LEN and int(a.streams[0]["recs"][-1]["status"]) == 1


@pytest.fixture(scope="module")
def mix():
    return SC.random_mix(20261021, 2000)


def test_random_mix_in_three_calls(gpu_ctx, mix):
    case = dict(name="mix", calls=mix, max_pages=0, frame_unstarted=False, flush=True)
    calls = run_case(gpu_ctx, case)
    every = [d for _, want in calls for d in want]
    assert {d["state"] for d in every} >= {SM.SYNCED, SM.NONE, SM.NOSTART, SM.NOT_TLS, SM.LOST, SM.CLOSED}
    assert sum(d["tail_in"] > 0 and d["entries"] != [] for d in every) > 200
    assert len({x for res, _ in calls for x in res.snis()}) > 400


def one_call(ctx, pk, max_packets=None, **kw):
    ts = flows.TLSStreams(ctx, configs.device_parser(SC.PARSER), max_packets or len(pk) + 8, **kw)
    res = ts.feed(*upload(pk))
    return ts, res


def test_capacity_rules_and_retry(gpu_ctx):
    """Zero, one short in each arena and exact: whole streams or nothing,
    nothing at or past a capacity, as the host twin; decode_all's retry gets
    everything."""
    pk = [f for i in range(70) for f in SC.conn(i, SC.flight(b"cap%d.example" % i) + C.rec(C.APP, bytes(50))[:7 + i % 9],
                                                [70 + i])]
    ts, res = one_call(gpu_ctx, pk)
    need = flows.TLSStreamDecoder.needed(res.counts)
    assert need[0] == 210 and need[1] == 70 and min(need) > 0
    full = device_again(ts, need)
    assert not int(full["counts"][5]) and not np.any(full["streams"][:70]["status"])
    trials = [(0, 0, 0, 0), tuple(x // 2 for x in need)]
    for k in range(4):
        trials.append(tuple(x - (j == k) for j, x in enumerate(need)))
    for caps in trials:
        dv, h = device_again(ts, caps), host_twin(ts, caps)
        assert_same_streams(h, dv, "caps %r" % (caps,))
        assert int(dv["counts"][5]) == 1 and flows.TLSStreamDecoder.needed(dv["counts"]) == need
        st = dv["streams"][:70]
        dropped = (st["status"] & _lib.TLSS_ST_DROPPED) != 0
        assert dropped.any() and list(st["state"]) == list(full["streams"][:70]["state"])
        for t in st[~dropped]:
            a, b = int(t["rec0"]), int(t["rec0"]) + int(t["nrec"])
            assert b <= caps[0] and dv["recs"][a:b].tobytes() == full["recs"][a:b].tobytes()
    last = ts.asm._last
    out = ts.decoder.decode_all(ts.ctx, ts.parser, last["data"], last["offsets"], last["caplens"], last["records"],
                                last["layouts"], last["out"], 1, 1, 1, 1, carry=ts._last_call["carry"])
    torch.cuda.synchronize()
    assert not int(out["counts"][5].item())
    for k, dt in (("recs", _lib.TLS_STREAM_REC_DTYPE), ("hellos", _lib.TLS_HELLO_DTYPE), ("snis", np.uint8), ("tails", np.uint8)):
        assert out[k].cpu().numpy().tobytes() == full[k].tobytes(), k
    ts.close()


def test_one_decoder_serves_calls_of_different_sizes(gpu_ctx):
    dec = flows.TLSStreamDecoder(2000)
    for n in (300, 5, 120):
        pk = [f for i in range(n) for f in SC.conn(i, SC.flight(b"n%d.example" % i), [50 + i % 100])]
        ts, res = one_call(gpu_ctx, pk)
        need = flows.TLSStreamDecoder.needed(res.counts)
        assert_same_streams(host_twin(ts, need), device_again(ts, need, decoder=dec), "n=%d" % n)
        assert len(res.snis()) == n
        ts.close()
    small = flows.TLSStreamDecoder(4)
    with pytest.raises(_lib.GpkError):
        device_again(ts, need, decoder=small)
    small.close()
    dec.close()


def test_stream_and_device_are_left_alone(gpu_ctx):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    before = torch.cuda.current_device()
    pk = [f for i in range(40) for f in SC.conn(i, SC.flight(), [90])]
    ts, res = one_call(gpu_ctx, pk)
    need = flows.TLSStreamDecoder.needed(res.counts)
    dec = flows.TLSStreamDecoder(len(pk) + 8, before)
    assert_same_streams(host_twin(ts, need), device_again(ts, need, decoder=dec, stream=torch.cuda.Stream()), "stream")
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = flows.TLSStreamDecoder(16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    dec.close()
    ts.close()
    assert torch.cuda.current_device() == before


def test_argument_faults(gpu_ctx):
    pk = SC.conn(1, SC.flight(), [50])
    ts, res = one_call(gpu_ctx, pk)
    last = ts.asm._last
    args = (ts.ctx, ts.parser, last["data"], last["offsets"], last["caplens"], last["records"], last["layouts"])
    good = ts.decoder.decode(*args, last["out"], 8, 4, 64, 64)
    torch.cuda.synchronize()
    assert good["counts"].cpu().tolist()[:6] == [1, 1, 3, 0, 1, 0]
    odd = dict(good, recs=good["recs"][4:])
    with pytest.raises(_lib.GpkError):
        ts.decoder.decode(*args, last["out"], 4, 4, 64, 64, out=odd)
    with pytest.raises(_lib.GpkError):
        ts.decoder.decode(*args, dict(last["out"], counts=None), 8, 4, 64, 64)
    n = last["offsets"].numel()
    bad = (torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
           torch.zeros(n + 1, dtype=torch.int32, device="cuda"), None)
    with pytest.raises(_lib.GpkError):
        ts.decoder.decode(*args, last["out"], 8, 4, 64, 64, carry=bad)
    ts.close()


def test_snilist_streams(gpu_ctx, tmp_path):
    """examples/snilist.py --streams over a pcap of split ClientHellos: every
    stream's name, where the per-packet listing finds two."""
    pk = CASES["split_one_call"]["calls"][0] + CASES["port_table"]["calls"][0]
    path = tmp_path / "split.pcap"
    with open(path, "wb") as f:
        f.write(struct.pack("<IHHiIII", 0xa1b2c3d4, 2, 4, 0, 0, 65535, 1))
        for i, p in enumerate(pk):
            f.write(struct.pack("<IIII", 1700000000 + i, 0, len(p), len(p)) + p)
    spec = importlib.util.spec_from_file_location("snilist", os.path.join(ROOT, "examples", "snilist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    got = mod.run(str(path), streams=True, batch=400, log=lines.append, ctx=gpu_ctx,
                  parser=configs.device_parser(SC.PARSER))
    model = SM.Streaming(SC.PARSER)
    want = {}
    for at in range(0, len(pk), 400):
        for g, name in names_of(model.feed(pk[at:at + 400])):
            want.setdefault(name, set()).add(g)
    for g, name in names_of(model.flush_all()):
        want.setdefault(name, set()).add(g)
    n = len(SC.flight()) - 1
    assert {k: v[1] for k, v in got.items()} == {k: len(v) for k, v in want.items()}
    assert got[b"split.example"] == [n, n] and got[b"alt.example"] == [1, 1] and b"web.example" not in got
    assert len(lines) == 2
    plain = mod.run(str(path), device=True, batch=400, log=lambda s: None)
    assert plain[b"split.example"][0] == 2  # per packet: only the cuts on a record boundary
