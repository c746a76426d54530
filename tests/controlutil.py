"""Helpers shared by the control-layer tests (CPU and GPU)."""
import json
import os

import numpy as np

import configs
import control_model as M
import controlcases as C
from gopacket_amd import flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import err_text, oracle_decoder  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "control_vectors.json")))["vectors"]
FIELD_OF = dict(contents="contents_len", payload="payload_len", next="next_type", err="err", a0="err_a0", a1="err_a1",
                status="status", unsupported="unsupported", id="id", seq="seq", typecode="typecode", hdr="hdr_off",
                op="arp_operation", hw="arp_hw_size", prot="arp_prot_size")


def decode_and_model(cfg, packets, kinds=15, checksum=True, align=1, pad=0, fill=0):
    """(model outputs, (data, offsets, caplens, oracle results)) of a packet list."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    m = M.control(cfg, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], kinds, checksum, fill=fill)
    return m, (data, offs, caps, ref)


def model_and_host(cfg, packets, kinds=15, checksum=True, align=1, pad=0, fill=0):
    m, (data, offs, caps, ref) = decode_and_model(cfg, packets, kinds, checksum, align, pad, fill)
    h = flows.ControlDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], configs.device_parser(cfg),
                                         kinds, checksum, fill=fill)
    return m, h, (data, offs, caps, ref)


def assert_same_control(m, h, what=""):
    """Every output array, record byte for record byte (entries past counts[0] included: they keep the fill)."""
    for k in flows.ControlDecoder.KEYS:
        if k == "records":
            bad = [j for j in range(len(m[k])) if m[k][j].tobytes() != h[k][j].tobytes()]
            assert not bad, "%s: control records differ at entries %s: model %s got %s" % (
                what, bad[:5], m[k][bad[:2]], h[k][bad[:2]])
        else:
            assert np.array_equal(m[k], h[k]), "%s: %s differs: model %s got %s" % (what, k, m[k], h[k])


def control_parser(cfg=C.PARSER, controls=(L.ICMPv4, L.ICMPv6, L.ICMPv6Echo, L.ARP), tunnels=()):
    """A DecodingLayerParser of `cfg` with the control (and tunnel) layers added
    and the decode oracle in place of the device."""
    by_name = dict(ETHERNET=L.Ethernet, DOT1Q=L.Dot1Q, IPV4=L.IPv4, IPV6=L.IPv6, IPV6_EXT=L.IPv6ExtensionSkipper,
                   TCP=L.TCP, UDP=L.UDP, PAYLOAD=G.Payload)
    p = G.DecodingLayerParser(cfg["first"], *[by_name[d]() for d in cfg["decoders"]])
    for t in tuple(controls) + tuple(tunnels):
        p.AddDecodingLayer(t())
    p.IgnoreUnsupported = bool(cfg.get("ignore_unsupported"))
    p._overrides = dict(ethertype=list((cfg.get("ethertype") or {}).items()), ipprotocol=[], tcp_port=[], udp_port=[])
    p._host_decoder = oracle_decoder(cfg)
    return p


def kinds_of(controls):
    k = 0
    for c in controls:
        k |= c.control_kind
    return k
