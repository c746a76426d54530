"""DNS over reassembled streams on the device (include/gpk_dns_streams.h):
flows.DNSStreams (TCPAssembler, then gpk_dns_streams) against the model
(dnsstream_model.py) field for field, and gpk_dns_streams against its host twin
byte for byte on the device's own reassembly, for every case of
dnsstreamcases.py: every split position in one call and in two, pointers across
the seam, the largest message, Length 0 and 11, the work cap, loss, close, no
SYN, the server direction, the port table, a carried final state, block and wave
edges of the per-stream and of the per-message kernels; a seeded mix in three
calls; both capacity retries; handle reuse, stream and device. No message here
carries a pointer chain longer than a few hundred bytes."""
import numpy as np
import pytest
import torch

import configs
import dns_model as M
import dnsstream_model as SM
import dnsstreamcases as SC
from dnsstreamutil import ARENAS, assert_same_streams, mix_case
from gopacket_amd import _lib, flows, layers as L
from pktutil import pack

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in SC.cases()}
SPARE = (3, 2, 5, 7)
D = flows.DNSStreamDecoder
SIZES = (80, 96, 1, 1)  # bytes per entry of msgs, rrs, names, tails
DTYPES = (_lib.DNS_STREAM_MSG_DTYPE, _lib.DNS_RR_DTYPE, np.uint8, np.uint8)


def upload(packets):
    data, offs, caps = pack(packets)
    d = torch.from_numpy(np.concatenate([data, np.zeros(-len(data) % 16 + 16, np.uint8)])).cuda()
    return d, torch.from_numpy(offs.astype(np.int64)).cuda(), torch.from_numpy(caps.astype(np.int32)).cuda()


def host_arrays(ts):
    """The arrays the last gpk_dns_streams call of `ts` worked on, on the host."""
    last = ts.asm._last
    o = last["out"]
    asm = {k: o[k].cpu().numpy() for k in ("stream_first", "stream_closed", "stream_data0", "counts", "data")}
    asm["chunks"] = o["chunks"].cpu().numpy().view(_lib.TCP_CHUNK_DTYPE)
    carry = tuple(None if t is None else t.cpu().numpy() for t in ts._last_call["carry"])
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
               counts=torch.full((12,), -1, dtype=torch.int64, device="cuda"))
    for k, c, sz in zip(ARENAS, caps, SIZES):
        out[k] = torch.full((c * sz,), fill, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    (decoder or ts.decoder).decode(ts.ctx, ts.parser, last["data"], last["offsets"], last["caplens"], last["records"],
                                   last["layouts"], last["out"], *caps, carry=ts._last_call["carry"],
                                   frame_unstarted=ts.frame_unstarted, max_message=ts.max_message, out=out, stream=stream)
    torch.cuda.synchronize()
    got = dict(streams=out["streams"].cpu().numpy().view(_lib.DNS_STREAM_DTYPE),
               counts=out["counts"].cpu().numpy().view(np.uint64))
    for k, dt in zip(ARENAS, DTYPES):
        got[k] = out[k].cpu().numpy().view(dt)
    return got


def host_twin(ts, caps, fill=0xA5):
    data, offs, cl, rec, lay, asm, carry = host_arrays(ts)
    return D.decode_host(ts.parser, data, offs, cl, rec, lay, asm, *caps, carry=carry,
                         frame_unstarted=ts.frame_unstarted, max_message=ts.max_message, fill=fill)


def same_layer(dns, m):
    """A hydrated layers.DNS against the model's message dict and the stream's bytes."""
    assert (dns.ID, dns.QDCount, dns.ANCount, dns.NSCount, dns.ARCount) == (m["id"], m["qdcount"], m["ancount"],
                                                                           m["nscount"], m["arcount"])
    assert int(dns.ResponseCode) == m["response_code"] and len(dns.Contents) == m["len"]
    got = dns.Questions + dns.Answers + dns.Authorities + dns.Additionals
    assert len(got) == len(m["rrs"])
    base = m["hdr_off"] if "hdr_off" in m else None
    for g, r in zip(got, m["rrs"]):
        assert g.Name == r["name"] and int(g.Type) == r["type"]
        if r["section"] == 0:
            continue
        assert g.DataLength == r["data_length"]
        if not r["data_length"]:  # decodeRData is skipped: no typed form
            continue
        if base is not None:  # Data is sliced from the stream's logical buffer
            at = r["data_off"] - base
            assert g.Data == dns.Contents[at:at + r["data_length"]]
        if r["type"] == SC.CNAME:
            assert g.CNAME == r["rname"]
        if r["type"] == SC.MX:
            assert (g.MX.Preference, g.MX.Name) == (r["v"][0], r["rname"])
        if r["type"] in (SC.A, SC.AAAA):
            assert g.IP == g.Data
        if r["type"] == SC.TXT:
            assert g.TXT == g.Data and len(g.TXTs) == r["count"]
        if r["type"] == SC.OPT:
            assert len(g.OPT) == r["count"]


def check_call(ts, res, want, what, hydrate=True):
    """One call: the wrapper's result against the model field for field, and
    the device against the host twin byte for byte, the arenas SPARE longer
    than needed (the device must leave those bytes alone)."""
    assert len(res.streams) == len(want), (what, len(res.streams), len(want))
    if not want:
        return
    for j, (s, d) in enumerate(zip(res.streams, want)):
        assert (s["id"], s["state"], s["tail_in"]) == (d["id"], d["state"], d["tail_in"]), (what, j, s, d)
        assert len(s["msgs"]) == len(d["entries"]), (what, j)
        for r, e in zip(s["msgs"], d["entries"]):
            assert (int(r["msg"]["hdr_off"]), int(r["status"]), int(r["present"]), int(r["stream"])) == (
                e["hdr_off"], e["mstatus"], e["present"], j), (what, j, r, e)
            assert int(r["msg"]["err"]) == e.get("err", 0) and int(r["msg"]["err_a0"]) == e.get("err_a0", 0)
            if "msg" in e:
                assert (int(r["msg"]["len"]), int(r["msg"]["id"]), int(r["msg"]["nrr"])) == (
                    e["len"], e["msg"]["id"], len(e["msg"]["rrs"]))
        assert (s["closed"] is not None) == d["closed"]
    assert res.questions() == SM.questions(want), what
    if hydrate:
        got, model = res.messages(), SM.decoded(want)
        assert [g for g, _ in got] == [g for g, _ in model], what
        for (_, dns), (_, m) in zip(got, model):
            assert isinstance(dns, L.DNS)
            same_layer(dns, dict(m, hdr_off=next(e["hdr_off"] for d in want for e in d["entries"] if e.get("msg") is m)))
    need = D.needed(res.counts)
    caps = tuple(a + b for a, b in zip(need, SPARE))
    dv, h = device_again(ts, caps), host_twin(ts, caps)
    assert_same_streams(h, dv, what)
    assert not int(dv["counts"][4]) and int(dv["counts"][0]) == len(want)
    # and the model's arrays: the same bytes (the host twin is held to them on the CPU)
    m = SM.to_arrays(want, len(dv["streams"]), caps, 0xA5)
    assert_same_streams(m, dv, what + " (model)")
    for e, d in zip(dv["streams"], want):  # the tails the model keeps are the bytes in the arena
        a = int(e["tail_off"])
        assert bytes(dv["tails"][a:a + int(e["tail_len"])]) == bytes(d["tail"]), what


def run_case(ctx, case, max_packets=None, hydrate=True):
    cfg = case["parser"]
    model = SM.Streaming(cfg, case["max_pages"], case["frame_unstarted"], case["max_message"])
    n = max(len(pk) for pk in case["calls"])
    ts = flows.DNSStreams(ctx, configs.device_parser(cfg), max_packets or n + 64, max_pages=case["max_pages"],
                          frame_unstarted=case["frame_unstarted"], max_message=case["max_message"])
    calls = []
    for k, pk in enumerate(case["calls"]):
        want = model.feed(pk)
        res = ts.feed(*upload(pk))
        check_call(ts, res, want, "%s call %d" % (case["name"], k), hydrate)
        calls.append((res, want))
    if case["flush"]:
        want = model.flush_all()
        res = ts.flush_all()
        check_call(ts, res, want, "%s flush" % case["name"], hydrate)
        calls.append((res, want))
    ts.close()
    return calls


@pytest.mark.parametrize("name", list(CASES))
def test_case(gpu_ctx, name):
    run_case(gpu_ctx, CASES[name])


@pytest.mark.parametrize("two", [False, True], ids=["one_call", "two_calls"])
def test_every_split_position(gpu_ctx, two):
    """One stream per cut position: every stream yields the query and the
    six-entry response, with a tail of one byte (half a prefix) and of two (a
    prefix, no body) among them."""
    calls = run_case(gpu_ctx, CASES["split_two_calls" if two else "split_one_call"])
    n = len(SC.exchange()) - 1
    got = {}
    for res, _ in calls:
        for s in res.streams:
            got.setdefault(s["id"], []).extend((int(r["msg"]["len"]), int(r["msg"]["nrr"]), int(r["msg"]["err"]))
                                               for r in s["msgs"])
    assert all(got[g] == [(29, 1, 0), (len(SC.response()), 7, 0)] for g in range(n))
    assert sorted(calls[-1][0].questions() + (calls[0][0].questions() if two else [])) == sorted(
        [(g, b"example.com", 1) for g in range(n)] * 2)
    if two:
        assert [s["tail_in"] for s in calls[1][0].streams][:3] == [1, 2, 3]


def test_seam_pointers_and_hydration(gpu_ctx):
    (_, _), (res, want) = run_case(gpu_ctx, CASES["seam_pointers"])
    assert [s["tail_in"] for s in res.streams] == [31, 18]
    for _, dns in res.messages():
        assert [a.Name for a in dns.Answers] == [b"example.com"] * 5
        assert dns.Answers[2].CNAME == b"www.example.com" and dns.Answers[3].MX.Name == b"mail.example.com"
        assert dns.Answers[0].IP == bytes([192, 0, 2, 1]) and dns.Answers[4].TXTs == [b"abc", b"hello"]
        assert len(dns.Additionals) == 1 and len(dns.Additionals[0].OPT) == 1


def test_largest_message_tail(gpu_ctx):
    calls = run_case(gpu_ctx, CASES["largest_message"])
    assert [len(w[0]["tail"]) for _, w in calls] == [20 * SC.MSS, _lib.DNSS_MAX_TAIL, 0]
    assert [int(r["msg"]["len"]) for r in calls[2][0].streams[0]["msgs"]] == [65535, 29]
    assert calls[2][0].streams[0]["tail_in"] == 65536


def test_states_by_hand(gpu_ctx):
    (a, _), (b, _) = run_case(gpu_ctx, CASES["page_limit_forces_a_skip"])  # LOST, then carried
    assert a.streams[0]["state"] == b.streams[0]["state"] == SM.LOST and len(b.streams[0]["msgs"]) == 0
    assert int(a.streams[0]["msgs"][-1]["status"]) == _lib.DNSS_MSG_PARTIAL
    ((a, _),) = run_case(gpu_ctx, CASES["length_0_and_11"])
    assert [int(r["msg"]["err"]) for r in a.streams[0]["msgs"]] == [M.E_SHORT, M.E_SHORT, 0]
    ((a, _),) = run_case(gpu_ctx, CASES["max_message"])
    assert [int(r["status"]) for r in a.streams[0]["msgs"]] == [0, _lib.DNSS_MSG_SKIPPED, 0]
    ((a, _),) = run_case(gpu_ctx, CASES["port_table"])
    assert [s["state"] for s in a.streams] == [SM.SYNCED, SM.NONE]


@pytest.fixture(scope="module")
def mix():
    return SC.random_mix(20261021, 2000)


def test_random_mix_in_three_calls(gpu_ctx, mix):
    calls = run_case(gpu_ctx, mix_case(mix))
    every = [d for _, want in calls for d in want]
    ents = [e for d in every for e in d["entries"]]
    assert {d["state"] for d in every} == {SM.SYNCED, SM.NONE, SM.NOSTART, SM.LOST, SM.CLOSED}
    assert 3 * sum("msg" in e for e in ents) >= len(ents) > 3000
    assert sum(d["tail_in"] > 0 and d["entries"] != [] for d in every) > 200


def one_call(ctx, pk, max_packets=None, **kw):
    ts = flows.DNSStreams(ctx, configs.device_parser(SC.PARSER), max_packets or len(pk) + 8, **kw)
    res = ts.feed(*upload(pk))
    return ts, res


def cap_packets(n):
    return [f for i in range(n) for f in SC.conn(i, SC.exchange(i) + SC.pre(SC.query())[:3 + i % 5], [40 + i % 30], dport=53)]


def test_capacity_rules_and_both_retries(gpu_ctx):
    """Zero, half, and one short in each arena: whole streams or nothing at
    level one, whole messages or nothing at level two, nothing at or past a
    capacity, as the host twin; decode_all's retries get everything."""
    ts, res = one_call(gpu_ctx, cap_packets(70))
    need = D.needed(res.counts)
    assert need[0] == 140 and need[1] == 70 * 8 and min(need) > 0
    full = device_again(ts, need)
    assert not int(full["counts"][4]) and not np.any(full["streams"][:70]["status"]) and not np.any(full["msgs"]["status"])
    trials = [(0, 0, 0, 0), tuple(x // 2 for x in need), (need[0], 0, 0, need[3])]
    for k in range(4):
        trials.append(tuple(x - (j == k) for j, x in enumerate(need)))
    for caps in trials:
        dv, h = device_again(ts, caps), host_twin(ts, caps)
        assert_same_streams(h, dv, "caps %r" % (caps,))
        assert int(dv["counts"][4]) == 1
        got = D.needed(dv["counts"])
        assert (got[0], got[3]) == (need[0], need[3])
        st = dv["streams"][:70]
        sdrop = (st["status"] & _lib.DNSS_ST_DROPPED) != 0
        placed = int(sum(int(t["nmsg"]) for t in st[~sdrop]))
        mdrop = (dv["msgs"][:placed]["status"] & _lib.DNSS_MSG_DROPPED) != 0
        assert sdrop.any() or mdrop.any()
        assert list(st["state"]) == list(full["streams"][:70]["state"])
        if not sdrop.any():
            assert got == need
        for e, f in zip(dv["msgs"][:placed][~mdrop], full["msgs"][:placed][~mdrop]):
            assert e.tobytes() == f.tobytes()
            a, b = int(e["msg"]["rr0"]), int(e["msg"]["rr0"]) + int(e["msg"]["nrr"])
            assert b <= caps[1] and dv["rrs"][a:b].tobytes() == full["rrs"][a:b].tobytes()
    last = ts.asm._last
    out = ts.decoder.decode_all(ts.ctx, ts.parser, last["data"], last["offsets"], last["caplens"], last["records"],
                                last["layouts"], last["out"], 1, 1, 1, 1, carry=ts._last_call["carry"])
    torch.cuda.synchronize()
    assert not int(out["counts"][4].item())
    for k, dt in zip(ARENAS, DTYPES):
        assert out[k].cpu().numpy().tobytes() == full[k].tobytes(), k
    ts.close()


def test_decoder_grows_with_the_messages(gpu_ctx):
    """More messages in a call than the decoder's scans hold: DNSStreams makes a larger one."""
    pk = SC.conn(1, SC.zone(1500), [700 * k for k in range(1, 60)], dport=53)
    ts, res = one_call(gpu_ctx, pk, max_packets=64)
    assert ts.decoder.max_msgs >= 1500 > 1024 and len(res.streams[0]["msgs"]) == 1500
    assert [q[1] for q in res.questions()[:2]] == [b"m0.zone.test", b"m1.zone.test"] and len(res.questions()) == 1500
    small = D(64, 16)
    with pytest.raises(_lib.GpkError):  # msg_cap > max_msgs
        device_again(ts, D.needed(res.counts), decoder=small)
    small.close()
    ts.close()


def test_one_decoder_serves_calls_of_different_sizes(gpu_ctx):
    dec = D(2000, 8000)
    for n in (300, 5, 120):
        pk = [f for i in range(n) for f in SC.conn(i, SC.exchange(i), [50 + i % 50], dport=53)]
        ts, res = one_call(gpu_ctx, pk)
        need = D.needed(res.counts)
        assert_same_streams(host_twin(ts, need), device_again(ts, need, decoder=dec), "n=%d" % n)
        assert len(res.questions()) == 2 * n
        ts.close()
    small = D(4)
    with pytest.raises(_lib.GpkError):
        device_again(ts, need, decoder=small)
    small.close()
    dec.close()


def test_stream_and_device_are_left_alone(gpu_ctx):
    """The call runs on the stream it is given and every entry restores the calling thread's device."""
    before = torch.cuda.current_device()
    pk = [f for i in range(40) for f in SC.conn(i, SC.exchange(i), [45], dport=53)]
    ts, res = one_call(gpu_ctx, pk)
    need = D.needed(res.counts)
    dec = D(len(pk) + 8, 256, before)
    assert_same_streams(host_twin(ts, need), device_again(ts, need, decoder=dec, stream=torch.cuda.Stream()), "stream")
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:  # a handle of another device
        other = D(16, 16, (before + 1) % torch.cuda.device_count())
        assert torch.cuda.current_device() == before
        other.close()
        assert torch.cuda.current_device() == before
    dec.close()
    ts.close()
    assert torch.cuda.current_device() == before


def test_argument_faults(gpu_ctx):
    pk = SC.conn(1, SC.exchange(), [50], dport=53)
    ts, res = one_call(gpu_ctx, pk)
    last = ts.asm._last
    args = (ts.ctx, ts.parser, last["data"], last["offsets"], last["caplens"], last["records"], last["layouts"])
    good = ts.decoder.decode(*args, last["out"], 8, 16, 256, 64)
    torch.cuda.synchronize()
    assert good["counts"].cpu().tolist()[:9] == [1, 1, 2, 0, 0, 2, 8, D.needed(res.counts)[2], 0]
    odd = dict(good, msgs=good["msgs"][4:])
    with pytest.raises(_lib.GpkError):
        ts.decoder.decode(*args, last["out"], 4, 16, 256, 64, out=odd)
    with pytest.raises(_lib.GpkError):
        ts.decoder.decode(*args, dict(last["out"], counts=None), 8, 16, 256, 64)
    with pytest.raises(_lib.GpkError):
        ts.decoder.decode(*args, last["out"], 8, 16, 256, 64, max_message=65536)
    n = last["offsets"].numel()
    bad = (torch.zeros(n + 1, dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
           torch.zeros(n + 1, dtype=torch.int32, device="cuda"), None)
    with pytest.raises(_lib.GpkError):
        ts.decoder.decode(*args, last["out"], 8, 16, 256, 64, carry=bad)
    ts.close()
