#!/usr/bin/env python3
"""What an IPv6 link says about itself: the neighbour table, the routers and
the multicast listeners of a capture.

A pcap or pcapng file is read in batches (pcapgo ReadBatch). Each batch is
decoded on the device by a DecodingLayerParser that holds the control layers
(ICMPv4, ICMPv6, ICMPv6Echo, ARP) and the ten NDP / MLD message layers: the
six-layer decode, the control pass (gpk_control_batch), then the NDP pass
(gpk_ndp_batch) over the packets whose ICMPv6 header leads to one of the ten.
Everything below is read from the passes' tables (the gpk_ndp records, their
gpk_ndp_entry descriptors, the gpk_control records of ARP) and the address and
option bytes those point at: no layer struct is hydrated.

  neighbours  IPv6 address -> link-layer address: the target of a Neighbor
              Advertisement with its Target Link-Layer Address option, and the
              IPv6 source of a Neighbor / Router Solicitation or Router
              Advertisement with its Source Link-Layer Address option; next to
              them the IPv4 pairs of the capture's ARP packets
  routers     per Router Advertisement source: lifetime, flags, the prefixes,
              the MTU and the RDNSS servers of its options
  listeners   per IPv6 source: the groups of its MLDv1 reports and of the
              records of its MLDv2 reports

  python examples/neighbors.py capture.pcap
"""
import argparse
import collections
import ipaddress
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ip(b):
    return str(ipaddress.ip_address(bytes(b)))


def _mac(b):
    return ":".join("%02x" % x for x in bytes(b))


def _source(res, i, pkt):
    """The IPv6 source address of packet i's innermost IPv6 header, from its layout slot; None without one."""
    from gopacket_amd import _lib
    part, pos = res._chain[i][-1]
    s = int(part.result.layouts[pos]["start"][_lib.DEC_IPV6 - 1])
    return None if s == 0xFFFFFFFF else pkt[s + 8:s + 24]


def run(inp, parser=None, device=True, batch=1 << 16, log=print):
    """Returns dict(neighbors={address: link-layer address}, arp={...},
    routers={source: dict(lifetime, flags, prefixes, mtu, rdnss)},
    listeners={source: [groups]}, messages, failed), every table in the order of
    first sight. parser: a DecodingLayerParser with the control and the NDP /
    MLD layers (default: the Ethernet one); device=False runs the host entries
    on the calling thread."""
    from gopacket_amd import _lib, gopacket as G, layers as L, pcapgo
    if parser is None:
        parser = G.DecodingLayerParser(L.LayerTypeEthernet, L.Ethernet(), L.Dot1Q(), L.IPv4(), L.IPv6(),
                                       L.IPv6ExtensionSkipper(), L.TCP(), L.UDP(), G.Payload(), L.ICMPv4(), L.ICMPv6(),
                                       L.ICMPv6Echo(), L.ARP(), *[c() for c in L.NDP_LAYERS])
    neighbors, arp = collections.OrderedDict(), collections.OrderedDict()
    routers, listeners = collections.OrderedDict(), collections.OrderedDict()
    messages = failed = 0
    with open(inp, "rb") as src:
        magic = src.read(4)
        src.seek(0)
        r = pcapgo.NewNgReader(src) if magic == b"\x0a\x0d\x0d\x0a" else pcapgo.NewReader(src)
        while True:
            try:
                b = r.ReadBatch(batch)
            except pcapgo.EOFErrorGo:
                break
            except pcapgo.PcapgoError as e:
                log("error getting packet: %s" % e)
                break
            pb = G.PacketBatch(b.data, b.offsets, b.caplens)
            res = parser.DecodeBatch(pb) if device else G.TunnelBatchResult(parser, pb, device=False)
            for i in range(len(pb)):
                c = res.Control(i)
                if c is not None and int(c["kind"]) == _lib.CTL_ARP and not int(c["err"]):
                    pkt = pb.packet(i)
                    a, hw, pr = int(c["hdr_off"]) + 8, int(c["arp_hw_size"]), int(c["arp_prot_size"])
                    if pr == 4:
                        arp.setdefault(_ip(pkt[a + hw:a + hw + pr]), _mac(pkt[a:a + hw]))
                    continue
                m = res.NDP(i)
                if m is None:
                    continue
                t, entries = m
                messages += 1
                if int(t["err"]):
                    failed += 1
                    continue
                pkt = pb.packet(i)
                lt = int(t["layer_type"])
                src6 = _source(res, i, pkt)
                opts = [(int(e["type"]), pkt[int(e["off"]):int(e["off"]) + int(e["ext"])]) for e in entries] \
                    if lt <= _lib.LT_ICMPV6_REDIRECT else []
                if lt == _lib.LT_ICMPV6_NEIGHBOR_ADVERTISEMENT:
                    target = pkt[int(t["v"][0]):int(t["v"][0]) + 16]
                    for typ, data in opts:
                        if typ == 2:
                            neighbors.setdefault(_ip(target), _mac(data))
                elif lt in (_lib.LT_ICMPV6_NEIGHBOR_SOLICITATION, _lib.LT_ICMPV6_ROUTER_SOLICITATION,
                            _lib.LT_ICMPV6_ROUTER_ADVERTISEMENT) and src6 is not None and any(src6):
                    for typ, data in opts:
                        if typ == 1:
                            neighbors.setdefault(_ip(src6), _mac(data))
                if lt == _lib.LT_ICMPV6_ROUTER_ADVERTISEMENT and src6 is not None:
                    ra = routers.setdefault(_ip(src6), dict(lifetime=0, flags=0, prefixes=[], mtu=None, rdnss=[]))
                    ra["lifetime"], ra["flags"] = int(t["v"][2]), int(t["flags"])
                    for typ, data in opts:
                        if typ == 3 and len(data) == 30:
                            p = "%s/%d" % (_ip(data[14:]), data[0])
                            if p not in ra["prefixes"]:
                                ra["prefixes"].append(p)
                        elif typ == 5 and len(data) == 6:
                            ra["mtu"] = int.from_bytes(data[2:], "big")
                        elif typ == 25:
                            for k in range(6, len(data) - 15, 16):
                                s = _ip(data[k:k + 16])
                                if s not in ra["rdnss"]:
                                    ra["rdnss"].append(s)
                groups = []
                if lt == _lib.LT_MLDV1_REPORT:
                    groups = [pkt[int(t["v"][0]):int(t["v"][0]) + 16]]
                elif lt == _lib.LT_MLDV2_REPORT:
                    groups = [pkt[int(e["off"]):int(e["off"]) + 16] for e in entries]
                if groups and src6 is not None:
                    seen = listeners.setdefault(_ip(src6), [])
                    for g in groups:
                        if _ip(g) not in seen:
                            seen.append(_ip(g))
    log("neighbours (%d NDP / MLD messages, %d failed)" % (messages, failed))
    for a, mac in neighbors.items():
        log("  %-40s %s" % (a, mac))
    for a, mac in arp.items():
        log("  %-40s %s  (arp)" % (a, mac))
    log("routers")
    for a, ra in routers.items():
        log("  %-40s lifetime %ds flags 0x%02x mtu %s" % (a, ra["lifetime"], ra["flags"], ra["mtu"]))
        for p in ra["prefixes"]:
            log("    prefix %s" % p)
        for s in ra["rdnss"]:
            log("    rdnss  %s" % s)
    log("listeners")
    for a, groups in listeners.items():
        log("  %-40s %s" % (a, " ".join(groups)))
    return dict(neighbors=neighbors, arp=arp, routers=routers, listeners=listeners, messages=messages, failed=failed)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("capture", help="a pcap or pcapng capture")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per batch")
    a = ap.parse_args()
    run(a.capture, batch=a.batch)


if __name__ == "__main__":
    main()
