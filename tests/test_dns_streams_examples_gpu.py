"""examples/dnstcp.py over a capture the test writes with pcapgo: DNS over TCP
streams whose messages span segments, a stream on a port that is no DNS port,
and UDP messages of the per-packet pass beside them. The listing is compared
with the models (dnsstream_model.py for the streams, dns_model.py for UDP)."""
import importlib.util
import os

import pytest

import configs
import dns_model as M
import dnscases as C
import dnsstream_model as SM
import dnsstreamcases as SC
from gopacket_amd import pcapgo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dnstcp_lists_streams_and_udp(gpu_ctx, tmp_path):
    tcp = [SC.conn(1, SC.exchange(0x1111), [10, 45], dport=53),                       # client side: split messages
           SC.conn(2, SC.pre(SC.response(0x2222)) + SC.zone(5), [30, 90], dport=50000, sport=53),  # server side
           SC.conn(3, SC.exchange(0x3333), [40], dport=80),                            # no DNS port
           SC.conn(4, SC.pre(SC.query(0x4444)) + SC.pre(bytes(11)), [20], dport=53, fin=True)]  # one message fails
    udp = [C.over(SC.query(0x5555)), C.over(SC.response(0x5555), sport=53, dport=50004), C.over(bytes(5))]
    pk = []
    for k in range(max(len(f) for f in tcp)):  # interleave the connections and the datagrams
        pk += [f[k] for f in tcp if k < len(f)] + udp[k:k + 1]
    path = tmp_path / "dnstcp.pcap"
    with open(path, "wb") as f:
        w = pcapgo.NewWriter(f)
        w.WriteFileHeader(65535, 1)
        for i, p in enumerate(pk):
            w.WritePacket(pcapgo.CaptureInfo((1700000000 + i, 0), len(p), len(p)), p)
    spec = importlib.util.spec_from_file_location("dnstcp", os.path.join(ROOT, "examples", "dnstcp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    batch = 7  # several batches: tails are carried between them
    got = mod.run(str(path), ctx=gpu_ctx, parser=configs.device_parser(SC.PARSER), batch=batch, log=lines.append)

    def row(m):
        return (bool(m["flags2"] & 0x80), m["id"], m["ancount"], [r["name"] for r in m["rrs"] if r["section"] == 0])
    model = SM.Streaming(SC.PARSER)
    want, failed = {}, 0
    for at in list(range(0, len(pk), batch)) + [None]:
        res = model.flush_all() if at is None else model.feed(pk[at:at + batch])
        for d in res:
            for e in d["entries"]:
                if "msg" in e:
                    want.setdefault(d["id"], []).append(row(e["msg"]))
                failed += "err" in e
    assert dict(got["streams"]) == want and got["failed"] == failed == 1
    assert sorted(len(v) for v in want.values()) == [1, 2, 6]  # the port-80 stream is no candidate
    wudp = []
    for i, p in enumerate(pk):
        if p in udp:
            try:
                wudp.append((i,) + row(M.decode_message(p[42:])))
            except M.GoError:
                pass
    assert got["udp"] == wudp and len(wudp) == 2
    assert sum(ln.startswith("tcp stream") for ln in lines) == 3 and "udp: 2 messages" in lines
    assert any("response     5 answers" in ln and "example.com" in ln for ln in lines)
