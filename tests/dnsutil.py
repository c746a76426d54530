"""Helpers shared by the DNS tests (CPU and GPU)."""
import json
import os

import numpy as np

import configs
import dns_model as M
import dnscases as C
from gopacket_amd import flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import err_text, oracle_decoder  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "dns_vectors.json")))["vectors"]


def golden_packet(v):
    """(Ethernet frame, offset of the message) of a harvested vector: bare
    messages and records ride in Ethernet / IPv4 / UDP to port 53, loopback
    frames get an Ethernet header in place of their four family bytes."""
    raw = bytes.fromhex(v["hex"])
    if v["link"] == "ethernet":
        return raw, v["at"]
    if v["link"] == "null":
        return C.MAC + (b"\x08\x00" if raw[4] >> 4 == 4 else b"\x86\xdd") + raw[4:], v["at"] + 10
    return C.over(raw), 42


def pcap_dns_frames():
    """The Ethernet / IPv4 / UDP frames of tests/golden/test_dns.pcap with port 53 on either side."""
    import struct
    import pktutil
    return [f for f in pktutil.read_pcap(pktutil.GOLDEN + "/test_dns.pcap")[1]
            if len(f) > 42 and f[12:14] == b"\x08\x00" and f[23] == 17 and 53 in struct.unpack(">HH", f[34:38])]


def decode_and_model(cfg, packets, align=1, pad=0, fill=0, rr_cap=None, name_cap=None):
    """(model outputs, (data, offsets, caplens, oracle results)) of a packet list."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    m = M.dns(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], rr_cap, name_cap, fill=fill)
    return m, (data, offs, caps, ref)


def model_and_host(cfg, packets, align=1, pad=0, fill=0, rr_cap=None, name_cap=None):
    m, (data, offs, caps, ref) = decode_and_model(cfg, packets, align, pad, fill, rr_cap, name_cap)
    h = flows.DNSDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], configs.device_parser(cfg),
                                     len(m["rrs"]), len(m["names"]), fill=fill)
    return m, h, (data, offs, caps, ref)


def assert_same_dns(m, h, what=""):
    """Every output array byte for byte (entries past counts[0] and past the
    capacities' use included: they keep the fill)."""
    for k in flows.DNSDecoder.KEYS:
        assert len(m[k]) == len(h[k]), (what, k, len(m[k]), len(h[k]))
        if k in ("records", "rrs"):
            bad = [j for j in range(len(m[k])) if m[k][j].tobytes() != h[k][j].tobytes()]
            assert not bad, "%s: %s differ at entries %s: model %s got %s" % (what, k, bad[:5], m[k][bad[:2]], h[k][bad[:2]])
        else:
            assert np.array_equal(m[k], h[k]), "%s: %s differs: model %s got %s" % (what, k, m[k], h[k])


def dns_parser(cfg=C.PARSER, extra=(L.DNS,), tunnels=()):
    """A DecodingLayerParser of `cfg` with layers.DNS (and further layers)
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
