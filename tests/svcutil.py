"""Helpers shared by the UDP service tests (CPU and GPU)."""
import json
import os

import numpy as np

import configs
import svc_model as M
import svccases as C
from gopacket_amd import flows, gopacket as G, layers as L
from pktutil import pack
from tunnelutil import err_text, oracle_decoder  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "svc_vectors.json")))
GOLDEN, GOLDEN_OPTIONS = _GOLDEN["vectors"], _GOLDEN["options"]
GOLDEN_PACKETS = [bytes.fromhex(v["hex"]) for v in GOLDEN]
CASES, EXPECT = C.quirk_cases()
NAMES = [n for n, _ in CASES]
PACKETS = [p for _, p in CASES]
FIELD_OF = dict(lt="layer_type", err="err", a0="err_a0", a1="err_a1", status="status", hdr="hdr_off", len="len",
                contents="contents_len", nentries="nentries")
CONTROLS = (L.ICMPv4, L.ICMPv6, L.ICMPv6Echo, L.ARP)
_corpus = []


def corpus():
    """The seeded corpus, built once."""
    if not _corpus:
        _corpus.extend(C.corpus(C.CORPUS_SEED, C.CORPUS_N, GOLDEN_PACKETS))
    return _corpus


def decode_and_model(cfg, packets, kinds=M.ALL, align=1, pad=0, fill=0, entry_cap=None):
    """(model outputs, (data, offsets, caplens, oracle results)) of a packet
    list; entry_cap None: exactly what the batch needs."""
    data, offs, caps = pack(packets, align=align, pad=pad)
    ref = configs.oracle_parser(cfg).decode(data, offs, caps)
    args = (cfg, data, offs, caps, ref["records"], ref["layouts"], kinds)
    if entry_cap is None:
        entry_cap = flows.ServiceDecoder.needed(M.svc(*args, entry_cap=0)["counts"])
    return M.svc(*args, entry_cap=entry_cap, fill=fill), (data, offs, caps, ref)


def model_and_host(cfg, packets, kinds=M.ALL, align=1, pad=0, fill=0, entry_cap=None):
    m, (data, offs, caps, ref) = decode_and_model(cfg, packets, kinds, align, pad, fill, entry_cap)
    h = flows.ServiceDecoder.decode_host(data, offs, caps, ref["records"], ref["layouts"], configs.device_parser(cfg),
                                         len(m["entries"]), kinds, fill=fill)
    return m, h, (data, offs, caps, ref)


def assert_same_svc(m, h, what=""):
    """Every output array whole (entries past counts[0] and past what the
    capacity let in included: they keep the fill)."""
    for k in flows.ServiceDecoder.KEYS:
        assert len(m[k]) == len(h[k]), (what, k, len(m[k]), len(h[k]))
        if k in ("records", "entries"):
            if m[k].tobytes() == h[k].tobytes():
                continue
            bad = [j for j in range(len(m[k])) if m[k][j].tobytes() != h[k][j].tobytes()]
            assert not bad, "%s: %s differ at entries %s: model %s got %s" % (what, k, bad[:5], m[k][bad[:2]], h[k][bad[:2]])
        else:
            assert np.array_equal(m[k], h[k]), "%s: %s differs: model %s got %s" % (what, k, m[k], h[k])


def device_arrays(out):
    """ServiceDecoder.decode's device tensors as the host entry's arrays."""
    from gopacket_amd import _lib
    return dict(verdict=out["verdict"].cpu().numpy(), class_start=out["class_start"].cpu().numpy().view(np.uint32),
                index=out["index"].cpu().numpy().view(np.uint32),
                records=out["records"].cpu().numpy().view(_lib.SVC_DTYPE),
                counts=out["counts"].cpu().numpy().view(np.uint32),
                entries=out["entries"].cpu().numpy().view(_lib.SVC_ENTRY_DTYPE))


def svc_parser(cfg=C.PARSER, extra=L.SVC_LAYERS, tunnels=()):
    """A DecodingLayerParser of `cfg` with the three service layers (and
    further ones) added and the decode oracle in place of the device."""
    by_name = dict(ETHERNET=L.Ethernet, DOT1Q=L.Dot1Q, IPV4=L.IPv4, IPV6=L.IPv6, IPV6_EXT=L.IPv6ExtensionSkipper,
                   TCP=L.TCP, UDP=L.UDP, PAYLOAD=G.Payload)
    p = G.DecodingLayerParser(cfg["first"], *[by_name[d]() for d in cfg["decoders"]])
    for t in tuple(extra) + tuple(tunnels):
        p.AddDecodingLayer(t())
    p.IgnoreUnsupported = bool(cfg.get("ignore_unsupported"))
    p._overrides = dict(ethertype=list((cfg.get("ethertype") or {}).items()), ipprotocol=[],
                        tcp_port=list((cfg.get("tcp_port") or {}).items()),
                        udp_port=list((cfg.get("udp_port") or {}).items()))
    p._host_decoder = oracle_decoder(cfg)
    return p
