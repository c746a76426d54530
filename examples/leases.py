#!/usr/bin/env python3
"""Who holds which IPv4 address: the DHCP leases, the DHCPv6 clients and the NTP
servers of a capture.

A pcap or pcapng file is read in batches (pcapgo ReadBatch). Each batch is
decoded on the device by a DecodingLayerParser that holds DHCPv4, DHCPv6 and
NTP: the six-layer decode, then the service pass (gpk_svc_batch) over the
packets whose UDP ports (or a table edit) lead to one of the three. Everything
below is read from the pass's tables (the gpk_svc records and their
gpk_svc_entry descriptors) and the address, name and option bytes those point
at: no layer struct is hydrated.

  clients   per client MAC (ClientHWAddr): the host name (option 12), the
            requested address (option 50) and the assigned one (YourClientIP
            of an Offer or Ack), the message types seen (option 53) in order,
            the server id (option 54), the lease time (option 51) and the
            vendor class (option 60)
  duids     per DHCPv6 transaction id: the client DUID bytes (option 1)
  ntp       per source of a server-mode (4) NTP message: stratum and version

  python examples/leases.py capture.pcap
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
    """The source address of packet i's innermost IP header, from its layout slots; None without one."""
    from gopacket_amd import _lib
    part, pos = res._chain[i][-1]
    lay = part.result.layouts[pos]
    s4, s6 = int(lay["start"][_lib.DEC_IPV4 - 1]), int(lay["start"][_lib.DEC_IPV6 - 1])
    if s6 != 0xFFFFFFFF and (s4 == 0xFFFFFFFF or s6 > s4):
        return pkt[s6 + 8:s6 + 24]
    return None if s4 == 0xFFFFFFFF else pkt[s4 + 12:s4 + 16]


def run(inp, parser=None, device=True, batch=1 << 16, log=print):
    """Returns dict(clients={mac: dict(hostname, requested, assigned, types,
    server, lease, vendor)}, duids={transaction id hex: DUID hex},
    ntp={source: dict(stratum, version)}, messages, failed), every table in the
    order of first sight. parser: a DecodingLayerParser with the three service
    layers (default: the Ethernet one); device=False runs the host entries on
    the calling thread."""
    from gopacket_amd import _lib, gopacket as G, layers as L, pcapgo
    if parser is None:
        parser = G.DecodingLayerParser(L.LayerTypeEthernet, L.Ethernet(), L.Dot1Q(), L.IPv4(), L.IPv6(),
                                       L.IPv6ExtensionSkipper(), L.TCP(), L.UDP(), G.Payload(), *[c() for c in L.SVC_LAYERS])
    clients, duids, ntp = collections.OrderedDict(), collections.OrderedDict(), collections.OrderedDict()
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
                m = res.Service(i)
                if m is None:
                    continue
                t, entries = m
                messages += 1
                if int(t["err"]):
                    failed += 1
                    continue
                pkt = pb.packet(i)
                lt, h = int(t["layer_type"]), int(t["hdr_off"])
                opts = [(int(e["code"]), pkt[int(e["off"]):int(e["off"]) + int(e["length"])]) for e in entries]
                if lt == _lib.LT_DHCPV4:
                    c = clients.setdefault(_mac(pkt[h + 28:h + 28 + int(t["b"][2])]),
                                           dict(hostname=None, requested=None, assigned=None, types=[], server=None,
                                                lease=None, vendor=None))
                    kind = next((d[0] for code, d in opts if code == int(L.DHCPOptMessageType) and len(d) == 1), None)
                    if kind is not None and L.DHCPMsgType(kind).String() not in c["types"]:
                        c["types"].append(L.DHCPMsgType(kind).String())
                    yiaddr = t["v"][3:4].astype("<u4").tobytes()
                    if kind in (int(L.DHCPMsgTypeOffer), int(L.DHCPMsgTypeAck)) and any(yiaddr):
                        c["assigned"] = _ip(yiaddr)
                    for code, d in opts:
                        if code == int(L.DHCPOptHostname):
                            c["hostname"] = d.decode("ascii", "replace")
                        elif code == int(L.DHCPOptRequestIP) and len(d) == 4:
                            c["requested"] = _ip(d)
                        elif code == int(L.DHCPOptServerID) and len(d) == 4:
                            c["server"] = _ip(d)
                        elif code == int(L.DHCPOptLeaseTime) and len(d) == 4:
                            c["lease"] = int.from_bytes(d, "big")
                        elif code == int(L.DHCPOptClassID):
                            c["vendor"] = d.decode("ascii", "replace")
                elif lt == _lib.LT_DHCPV6:
                    if int(t["b"][0]) not in (12, 13):
                        for code, d in opts:
                            if code == int(L.DHCPv6OptClientID):
                                duids.setdefault("%06x" % int(t["v"][0]), d.hex())
                elif int(t["b"][2]) == 4:  # NTP, server mode
                    s = _source(res, i, pkt)
                    if s is not None:
                        ntp.setdefault(_ip(s), dict(stratum=int(t["b"][3]), version=int(t["b"][1])))
    log("clients (%d DHCP / NTP messages, %d failed)" % (messages, failed))
    for mac, c in clients.items():
        log("  %s  %-20s requested %s assigned %s server %s lease %s vendor %s  [%s]" % (
            mac, c["hostname"], c["requested"], c["assigned"], c["server"], c["lease"], c["vendor"], " ".join(c["types"])))
    log("dhcpv6 transactions")
    for x, d in duids.items():
        log("  %s  client duid %s" % (x, d))
    log("ntp servers")
    for a, s in ntp.items():
        log("  %-40s stratum %d version %d" % (a, s["stratum"], s["version"]))
    return dict(clients=clients, duids=duids, ntp=ntp, messages=messages, failed=failed)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("capture", help="a pcap or pcapng capture")
    ap.add_argument("--batch", type=int, default=1 << 16, help="packets per batch")
    a = ap.parse_args()
    run(a.capture, batch=a.batch)


if __name__ == "__main__":
    main()
