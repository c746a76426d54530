"""examples/pcaprewrite.py (read a capture, decode with fields, rewrite the
fields with tensor operations, SerializeBatch with both options, WritePackets)
over a small generated pcap, in batches of 50 so its packets make several. The
output file is read back with the project's reader and must hold the model
(serialize_model.py) applied to the same rewrite of the oracle's fields."""
import importlib.util
import os
import struct

import numpy as np
import pytest

import serialize_model as M
import serializecases as C
from gopacket_amd import pcapgo as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD, NEW = "192.168.7.9", "172.16.0.99"


def example():
    spec = importlib.util.spec_from_file_location("pcaprewrite", os.path.join(ROOT, "examples", "pcaprewrite.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def packets():
    keep = ("pad_", "vlan", "qinq", "ip4_nop", "tcp_m", "hbh_", "6in4", "4in6", "ip4_in_ip4", "ip6_dest", "8023", "no_layers")
    pk = [p for (name, p, edit) in C.cases() if name.startswith(keep) and len(p) < 3000]
    pk += [C.tcp4(n, n) for n in (0, 1, 700, 1460)] + [C.udp6(n, n) for n in (0, 33, 1200)]
    pk += [C.eth(C.ip4(C.udp(C.blob(40, 2)), 17, dst=bytes([8, 8, 8, 8]), ttl=0), 0x0800)]  # not OLD; TTL 0 stays 0
    return pk


def model_rewrite(pk, dnat, ttl_dec, vlan_pop):
    data, off, cap = C.pack_at(pk, [0] * len(pk))
    lay, f = C.decode(data, off, cap)
    for r in f:
        p = int(r["present"])
        if dnat and p >> C.IP4 & 1 and bytes(r["ip4_dst"]) == bytes(int(x) for x in OLD.split(".")):
            r["ip4_dst"] = [int(x) for x in NEW.split(".")]
        if ttl_dec and p >> C.IP4 & 1 and r["ip4_ttl"] > 0:
            r["ip4_ttl"] -= 1
        if ttl_dec and p >> C.IP6 & 1 and r["ip6_hop_limit"] > 0:
            r["ip6_hop_limit"] -= 1
        if vlan_pop and p >> C.D1Q & 1 and p & 1:
            r["eth_type"] = r["d1q_type"]
            r["present"] = p & (0xFF ^ (1 << C.D1Q))
    ref = M.serialize_batch(data, off, cap, lay, f, None, 1, 1)
    return [bytes(ref["out"][int(ref["offsets"][j]):int(ref["offsets"][j + 1])]) if ref["status"][j] == 0 else None
            for j in range(len(pk))]


@pytest.mark.parametrize("dnat,ttl_dec,vlan_pop", [(True, True, True), (True, False, False), (False, False, True)])
def test_pcaprewrite(tmp_path, gpu_ctx, dnat, ttl_dec, vlan_pop):
    pk = packets()
    src = tmp_path / "in.pcap"
    with open(src, "wb") as f:
        f.write(struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1))
        for i, p in enumerate(pk):
            f.write(struct.pack("<IIII", 1700000000 + i, i * 7, len(p), len(p)) + p)
    want = model_rewrite(pk, dnat, ttl_dec, vlan_pop)
    assert any(w is None for w in want) and sum(w is not None and w != p for w, p in zip(want, pk)) > 10
    out = str(tmp_path / "out.pcap")
    read, written, rejected = example().run(str(src), out, (OLD, NEW) if dnat else None, ttl_dec, vlan_pop, batch=50,
                                            log=lambda s: None)
    kept = [(i, w) for i, w in enumerate(want) if w is not None]
    assert (read, written, rejected) == (len(pk), len(kept), len(pk) - len(kept))
    r = P.NewReader(open(out, "rb"))
    for i, w in kept:
        d, ci = r.ReadPacketData()
        assert d == w, i
        assert (ci.Timestamp, ci.CaptureLength, ci.Length) == ((1700000000 + i, i * 7000), len(w), len(w))
    with pytest.raises(EOFError):
        r.ReadPacketData()
