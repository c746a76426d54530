"""Helpers shared by the tunnel tests (CPU and GPU)."""
import json
import os

import numpy as np

import configs
import tunnel_model as M
import tunnelcases as C
from gopacket_amd import flows, gopacket as G, layers as L
from pktutil import pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "tunnel_vectors.json")))["vectors"]


def golden_packet(v):
    """(parser cfg, packet) of a harvested vector; bare GRE headers ride in Ethernet / IPv4."""
    raw = bytes.fromhex(v["hex"])
    if v.get("bare_header"):
        return C.PARSER, C.over_ip(raw), 34
    return dict(C.PARSER, first=v["first"]), raw[v["skip"]:], -v["skip"]


def model_and_host(cfg, packets, kinds=7, gre_checksum=True, align=1, pad=0, fill=0):
    data, offs, caps = pack(packets, align=align, pad=pad)
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    m = M.peel(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], kinds, gre_checksum, fill=fill)
    h = flows.Detunneler.peel_host(data, offs, caps, ref["records"], ref["layouts"], configs.device_parser(cfg), kinds,
                                   gre_checksum, fill=fill)
    return m, h, (data, offs, caps, ref)


def assert_same_peel(m, h, what=""):
    for k in flows.Detunneler.KEYS:
        if k == "tunnels":
            bad = [j for j in range(len(m[k])) if m[k][j].tobytes() != h[k][j].tobytes()]
            assert not bad, "%s: tunnel records differ at entries %s: model %s got %s" % (
                what, bad[:5], m[k][bad[:2]], h[k][bad[:2]])
        else:
            assert np.array_equal(m[k], h[k]), "%s: %s differs: model %s got %s" % (what, k, m[k], h[k])


def oracle_decoder(cfg):
    def dec(parser, data, offsets, caplens):
        return configs.oracle_parser(dict(cfg, first=int(parser.first))).decode(data, offsets, caplens)
    return dec


def tunnel_parser(cfg=C.PARSER, tunnels=(L.GRE, L.VXLAN, L.Geneve)):
    p = G.DecodingLayerParser(cfg["first"], L.Ethernet(), L.Dot1Q(), L.IPv4(), L.IPv6(), L.IPv6ExtensionSkipper(),
                              L.TCP(), L.UDP(), G.Payload())
    for t in tunnels:
        p.AddDecodingLayer(t())
    p.IgnoreUnsupported = bool(cfg.get("ignore_unsupported"))
    p._host_decoder = oracle_decoder(cfg)
    return p


def err_text(e):
    return "" if e is None else e.Error()


def check_composition(res, want, n):
    """A TunnelBatchResult against tunnel_model.compose: decoded, error text and
    Truncated per packet, then every level's parts, slices and records."""
    for i in range(n):
        assert [int(t) for t in res.Decoded(i)] == want["decoded"][i], i
        assert err_text(res.Err(i)) == want["error"][i], i
        assert res.Truncated(i) == want["truncated"][i], i
    # every level's record is the decode oracle's for that level's slices
    assert len(res.levels) == len(want["levels"])
    for k, parts in enumerate(res.levels):
        assert [int(x.first) for x in parts] == [x["first"] for x in want["levels"][k]]
        for part, w in zip(parts, want["levels"][k]):
            assert list(part.index) == w["origin"]
            assert [part.batch.packet(j) for j in range(len(part.index))] == w["packets"]
            configs.assert_same(dict(records=part.result.records, err_args=part.result.err_args,
                                     flows=part.result.flows, layouts=part.result.layouts), w["results"], "level %d" % k)
