"""Helpers shared by the TLS tests (CPU and GPU)."""
import json
import os

import numpy as np

import configs
import tls_model as M
import tlscases as C
from gopacket_amd import flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import err_text, oracle_decoder  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "tls_vectors.json")))["vectors"]
ENTRY_KEYS = ("records", "recs", "hellos")


def golden_packet(v):
    """(Ethernet frame, offset of the message) of a harvested vector: bare
    messages ride in Ethernet / IPv4 / TCP to port 443."""
    raw = bytes.fromhex(v["hex"])
    if v["link"] == "ethernet":
        return raw, v["at"]
    return C.over(raw), C.AT


def decode_and_model(cfg, packets, align=1, pad=0, fill=0, caps3=(None, None, None)):
    """(model outputs, (data, offsets, caplens, oracle results)) of a packet list."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    m = M.tls(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], *caps3, fill=fill)
    return m, (data, offs, caps, ref)


def model_and_host(cfg, packets, align=1, pad=0, fill=0, caps3=(None, None, None)):
    m, (data, offs, caps, ref) = decode_and_model(cfg, packets, align, pad, fill, caps3)
    h = flows.TLSDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], configs.device_parser(cfg),
                                     len(m["recs"]), len(m["hellos"]), len(m["snis"]), fill=fill)
    return m, h, (data, offs, caps, ref)


def assert_same_tls(m, h, what=""):
    """Every output array byte for byte (entries past counts[0] and past the
    capacities' use included: they keep the fill)."""
    for k in flows.TLSDecoder.KEYS:
        assert len(m[k]) == len(h[k]), (what, k, len(m[k]), len(h[k]))
        if k in ENTRY_KEYS:
            bad = [j for j in range(len(m[k])) if m[k][j].tobytes() != h[k][j].tobytes()]
            assert not bad, "%s: %s differ at entries %s: model %s got %s" % (what, k, bad[:5], m[k][bad[:2]], h[k][bad[:2]])
        else:
            assert np.array_equal(m[k], h[k]), "%s: %s differs: model %s got %s" % (what, k, m[k], h[k])


def tls_parser(cfg=C.PARSER, extra=(L.TLS,), tunnels=()):
    """A DecodingLayerParser of `cfg` with layers.TLS (and further layers)
    added and the decode oracle in place of the device."""
    by_name = dict(ETHERNET=L.Ethernet, DOT1Q=L.Dot1Q, IPV4=L.IPv4, IPV6=L.IPv6, IPV6_EXT=L.IPv6ExtensionSkipper,
                   TCP=L.TCP, UDP=L.UDP, PAYLOAD=G.Payload)
    p = G.DecodingLayerParser(cfg["first"], *[by_name[d]() for d in cfg["decoders"]])
    for t in tuple(extra) + tuple(tunnels):
        p.AddDecodingLayer(t())
    p.IgnoreUnsupported = bool(cfg.get("ignore_unsupported"))
    p._overrides = dict(ethertype=list((cfg.get("ethertype") or {}).items()), ipprotocol=[],
                        tcp_port=list((cfg.get("tcp_port") or {}).items()), udp_port=[])
    p._host_decoder = oracle_decoder(cfg)
    return p

