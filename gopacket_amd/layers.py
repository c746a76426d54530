"""gopacket/layers surface for the hot path: LayerType and enum constants and
the DecodingLayer structs Ethernet, Dot1Q, IPv4, IPv6, IPv6ExtensionSkipper,
TCP, UDP (layers/{ethernet,dot1q,ip4,ip6,tcp,udp}.go), and the three tunnel
layers GRE, VXLAN, Geneve (layers/{gre,vxlan,geneve}.go), which are filled from
the gpk_tunnel record of gpk_tunnel_batch (include/gpk_tunnel.h), and the four
control layers ICMPv4, ICMPv6, ICMPv6Echo, ARP (layers/{icmp4,icmp6,icmp6msg,
arp}.go), filled from the gpk_control record of gpk_control_batch
(include/gpk_control.h), and DNS (layers/dns.go), filled from the gpk_dns
record, the gpk_dns_rr entries and the name arena of gpk_dns_batch
(include/gpk_dns.h), and TLS (layers/tls*.go), filled from the gpk_tls record
and the gpk_tls_rec and gpk_tls_hello entries of gpk_tls_batch
(include/gpk_tls.h).

These structs are filled from device results, in one of two ways:
- _fill(pkt, s, e, f): from the gpk_fields record the device wrote for the
  packet (gpk_decode_batch_fields) and the slice [s, e) its DecodeFromBytes
  was handed (derived from the decoded list, gopacket.BatchResult.Hydrate):
  every scalar field is the record's, option lists come from the record's
  option start maps, and Contents/Payload are slices at the header length and
  payload end the record's fields give. No header is decoded on the host.
- _hydrate(d): from the slice alone (a gpk_layout range), every field a pure
  read of those packet bytes, following the field assignments of the
  reference decoder it names; the fallback for what the record does not hold.
Option lists are walked from bytes whose validity the device already
established (the device reports any option error as the packet's error).
"""
import json
import os
import struct
from dataclasses import dataclass, field
from typing import List, Optional

from . import _lib
from .gopacket import (ChecksumVerificationResult, Flow, LayerClass, LayerType, NewFlow, EndpointIPv4, EndpointIPv6,
                       EndpointMAC, EndpointTCPPort, EndpointUDPPort, EndpointSCTPPort, EndpointRUDPPort,
                       EndpointUDPLitePort, EndpointPPP, InvalidEndpoint, NewEndpoint, LayerTypeFragment,
                       LayerTypePayload)

_REG = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "registry_gen.json")))

# ---- LayerType constants (layers/layertypes.go) -----------------------------
_by_name = {}
for _id, _name in _REG["layer_type_names"].items():
    _by_name.setdefault(_name, int(_id))


def _lt(name):
    return LayerType(_by_name[name])


LayerTypeARP = _lt("ARP")
LayerTypeDot1Q = _lt("Dot1Q")
LayerTypeEthernet = _lt("Ethernet")
LayerTypeICMPv4 = _lt("ICMPv4")
LayerTypeIPv4 = _lt("IPv4")
LayerTypeIPv6 = _lt("IPv6")
LayerTypeLLC = _lt("LLC")
LayerTypeTCP = _lt("TCP")
LayerTypeUDP = _lt("UDP")
LayerTypeIPv6HopByHop = _lt("IPv6HopByHop")
LayerTypeIPv6Routing = _lt("IPv6Routing")
LayerTypeIPv6Fragment = _lt("IPv6Fragment")
LayerTypeIPv6Destination = _lt("IPv6Destination")
LayerTypeDNS = _lt("DNS")
LayerTypeTLS = _lt("TLS")
LayerTypeModbus = _lt("Modbus")
LayerTypeENIP = _lt("ENIP")
LayerTypeGRE = _lt("GRE")
LayerTypeVXLAN = _lt("VXLAN")
LayerTypeGeneve = _lt("Geneve")
LayerTypeICMPv6 = _lt("ICMPv6")
LayerTypeICMPv6RouterSolicitation = _lt("ICMPv6RouterSolicitation")
LayerTypeICMPv6RouterAdvertisement = _lt("ICMPv6RouterAdvertisement")
LayerTypeICMPv6NeighborSolicitation = _lt("ICMPv6NeighborSolicitation")
LayerTypeICMPv6NeighborAdvertisement = _lt("ICMPv6NeighborAdvertisement")
LayerTypeICMPv6Redirect = _lt("ICMPv6Redirect")
LayerTypeICMPv6Echo = _lt("ICMPv6Echo")
LayerTypeMLDv1MulticastListenerReport = _lt("MLDv1MulticastListenerReport")
LayerTypeMLDv1MulticastListenerDone = _lt("MLDv1MulticastListenerDone")
LayerTypeMLDv1MulticastListenerQuery = _lt("MLDv1MulticastListenerQuery")
LayerTypeMLDv2MulticastListenerReport = _lt("MLDv2MulticastListenerReport")
LayerTypeMLDv2MulticastListenerQuery = _lt("MLDv2MulticastListenerQuery")
# layertypes.go:200-206
LayerClassIPv6Extension = LayerClass([LayerTypeIPv6HopByHop, LayerTypeIPv6Routing, LayerTypeIPv6Fragment,
                                      LayerTypeIPv6Destination])

# ---- enums (layers/enums.go) -------------------------------------------------
EthernetTypeLLC = 0x0000
EthernetTypeIPv4 = 0x0800
EthernetTypeARP = 0x0806
EthernetTypeIPv6 = 0x86DD
EthernetTypeDot1Q = 0x8100
EthernetTypeQinQ = 0x88A8
IPProtocolIPv6HopByHop = 0
IPProtocolTCP = 6
IPProtocolUDP = 17
IPProtocolIPv4 = 4
IPProtocolIPv6 = 41
IPProtocolNoNextHeader = 59
IPv6HopByHopOptionJumbogram = 0xC2

_IPPROTO_NAMES = {v: n for v, lt, n in _REG["ipprotocol"]}
_ETHERTYPE_NAMES = {v: n for v, lt, n in _REG["ethertype"]}


def IPProtocolString(p):
    """IPProtocol.String() (enums_generated.go:135-143)"""
    return IPProtocolMetadata._name(int(p))


def EthernetTypeString(t):
    """EthernetType.String() (enums_generated.go:65-73)"""
    return EthernetTypeMetadata._name(int(t))


# ---- next-layer tables (layers/enums.go:294-390, ports.go:54-183) -----------
# The registry the reference's NextLayerType methods consult, as the host
# mirror: EthernetTypeMetadata / IPProtocolMetadata (EnumMetadata per value,
# enums.go:294-353, editable as in Go) and the TCP/UDP port overrides of
# RegisterTCPPortLayerType / RegisterUDPPortLayerType (ports.go:95-104,
# 174-183) over the port switches. Every DecodingLayerParser built after an
# edit sends the edited entries to its device parser (gpk_parser_set_*), so
# the device's NextLayerType lookups and the structs' NextLayerType() agree.


class EnumMetadata:
    """enums.go EnumMetadata: the decoder, the name and the LayerType of a
    value. Go's EthernetType / IPProtocol LayerType() and String() read an
    entry only when its DecodeWith is set (enums_generated.go:65-84,
    135-154): an entry written without one decodes as nothing (LayerType 0)
    and prints as unknown, whatever its LayerType and Name say."""

    def __init__(self, LayerType=0, Name="", DecodeWith=None):
        self.LayerType, self.Name, self.DecodeWith = LayerType, Name, DecodeWith

    def __repr__(self):
        return "EnumMetadata(LayerType=%d, Name=%r, DecodeWith=%r)" % (int(self.LayerType), self.Name,
                                                                       self.DecodeWith)


class _GoDecoder:
    """The DecodeWith of an entry initActualTypeData registered (enums.go:310-353):
    a decoder of the reference's NewPacket path, which the hot path never calls."""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "decode%s" % self.name


class _EnumTable:
    """A [n]EnumMetadata array: the generated defaults, and every entry a
    caller has touched kept as its own object, so both forms of Go's edit
    work: `T[v] = EnumMetadata(...)` and `T[v].LayerType = ...`."""

    def __init__(self, rows, n, unknown):
        self._default = {v: (LayerType(lt), name) for v, lt, name in rows}
        self._n, self._unknown, self._edits = n, unknown, {}

    def _effective(self, v):
        """What Go's LayerType() returns for v (0 without a DecodeWith)."""
        m = self._edits.get(v)
        if m is None:
            return int(self._default.get(v, (0, ""))[0])
        return int(m.LayerType) if m.DecodeWith is not None else 0

    def _name(self, v):
        m = self[v]
        return m.Name if m.DecodeWith is not None else self._unknown

    def _check(self, v):
        v = int(v)
        if not 0 <= v < self._n:
            raise IndexError(v)
        return v

    def __getitem__(self, v):
        v = self._check(v)
        if v not in self._edits:
            if v in self._default:
                lt, name = self._default[v]
                self._edits[v] = EnumMetadata(lt, name, _GoDecoder(name))
            else:  # the zero EnumMetadata: no decoder
                self._edits[v] = EnumMetadata(LayerType(0), "", None)
        return self._edits[v]

    def __setitem__(self, v, meta):
        self._edits[self._check(v)] = meta

    def _changed(self):
        """(value, LayerType) of every entry whose effective LayerType differs from the default."""
        out = []
        for v in sorted(self._edits):
            lt = self._effective(v)
            if lt != int(self._default.get(v, (0, ""))[0]):
                out.append((v, lt))
        return out


EthernetTypeMetadata = _EnumTable(_REG["ethertype"], 65536, "UnknownEthernetType")
IPProtocolMetadata = _EnumTable(_REG["ipprotocol"], 256, "UnknownIPProtocol")

_TCP_SWITCH = {p: LayerType(lt) for p, lt in _REG["tcp_port_switch"]}
_UDP_SWITCH = {p: LayerType(lt) for p, lt in _REG["udp_port_switch"]}
_tcp_override = {p: LayerType(lt) for p, lt in _REG["tcp_port_override"]}  # init() registrations
_udp_override = {p: LayerType(lt) for p, lt in _REG["udp_port_override"]}
_tcp_user, _udp_user = {}, {}


def RegisterTCPPortLayerType(port, layerType):
    """ports.go:99-104"""
    _tcp_override[int(port)] = _tcp_user[int(port)] = LayerType(layerType)


def RegisterUDPPortLayerType(port, layerType):
    """ports.go:178-183"""
    _udp_override[int(port)] = _udp_user[int(port)] = LayerType(layerType)


def EthernetTypeLayerType(t):
    """EthernetType.LayerType() (enums_generated.go:76-84)."""
    return LayerType(EthernetTypeMetadata._effective(EthernetTypeMetadata._check(t)))


def IPProtocolLayerType(p):
    """IPProtocol.LayerType() (enums_generated.go:146-154)."""
    return LayerType(IPProtocolMetadata._effective(IPProtocolMetadata._check(p)))


def TCPPortLayerType(port):
    """TCPPort.LayerType() (ports.go:54-93): the override, else the switch, else Payload."""
    port = int(port)
    if port in _tcp_override:
        return _tcp_override[port]
    return _TCP_SWITCH.get(port, LayerTypePayload)


def UDPPortLayerType(port):
    """UDPPort.LayerType() (ports.go:121-172)."""
    port = int(port)
    if port in _udp_override:
        return _udp_override[port]
    return _UDP_SWITCH.get(port, LayerTypePayload)


def _reset_registry():
    """Back to the reference's registry after init() (tests)."""
    EthernetTypeMetadata._edits.clear()
    IPProtocolMetadata._edits.clear()
    _tcp_user.clear()
    _udp_user.clear()
    _tcp_override.clear()
    _tcp_override.update({p: LayerType(lt) for p, lt in _REG["tcp_port_override"]})
    _udp_override.clear()
    _udp_override.update({p: LayerType(lt) for p, lt in _REG["udp_port_override"]})


def _registry_edits():
    """What a device parser must be told beyond its default tables."""
    return dict(ethertype=EthernetTypeMetadata._changed(), ipprotocol=IPProtocolMetadata._changed(),
                tcp_port=sorted((p, int(lt)) for p, lt in _tcp_user.items()),
                udp_port=sorted((p, int(lt)) for p, lt in _udp_user.items()))


def _be16(b, o):
    return (b[o] << 8) | b[o + 1]


def _be32(b, o):
    return struct.unpack_from(">I", b, o)[0]


_NO_DECODER = 1999  # a LayerType no device parser has a decoder for


def _tables_into(own):
    """(value, LayerType) entries that send every next-layer lookup landing on
    one of the types in `own` to a type without a decoder instead."""
    def enum(t):
        vals = set(t._default) | set(t._edits)
        return [(v, _NO_DECODER) for v in sorted(vals) if t._effective(v) in own]

    def ports(switch, override, lookup):
        return [(p, _NO_DECODER) for p in sorted(set(switch) | set(override)) if int(lookup(p)) in own]

    return dict(ethertype=enum(EthernetTypeMetadata), ipprotocol=enum(IPProtocolMetadata),
                tcp_port=ports(_TCP_SWITCH, _tcp_override, TCPPortLayerType),
                udp_port=ports(_UDP_SWITCH, _udp_override, UDPPortLayerType))


class BaseLayer:
    Contents: bytes = b""
    Payload: bytes = b""

    def LayerContents(self):
        return self.Contents

    def LayerPayload(self):
        return self.Payload

    def DecodeFromBytes(self, data, df):
        """The DecodingLayer method (ethernet.go:42-63, dot1q.go:30-41,
        ip4.go:178-271, ip6.go:221-278, 443-451, tcp.go:291-551, udp.go:30-56),
        on the device: one packet through a parser holding only this layer,
        whose next-layer tables lead nowhere back into it, so exactly this one
        header is decoded. Returns the decoder's error (None on success); a
        truncated header calls df.SetTruncated(); a decoder panic raises
        GoPanic, as it propagates out of DecodeFromBytes in Go."""
        from .gopacket import DecodingLayerArray, _LayersDecoder
        types = self.CanDecode().LayerTypes()
        dec = _LayersDecoder(DecodingLayerArray().Put(self), types[0], df, _tables_into({int(t) for t in types}))
        _, err = dec(bytes(data), [])
        return err


# ---- layers/ethernet.go:22-63 ------------------------------------------------
class Ethernet(BaseLayer):
    kind = _lib.DEC_ETHERNET

    def __init__(self):
        self.SrcMAC = self.DstMAC = b""
        self.EthernetType = 0
        self.Length = 0

    def LayerType(self):
        return LayerTypeEthernet

    def CanDecode(self):
        return LayerClass([LayerTypeEthernet])

    def _hydrate(self, d):
        self.DstMAC = d[0:6]
        self.SrcMAC = d[6:12]
        self.EthernetType = _be16(d, 12)
        self.Contents, self.Payload = d[:14], d[14:]
        self._poff = 14
        self.Length = 0
        if self.EthernetType < 0x0600:
            self.Length = self.EthernetType
            self.EthernetType = EthernetTypeLLC
            if len(self.Payload) > self.Length:
                self.Payload = self.Payload[:self.Length]

    def _fill(self, pkt, s, e, f):
        self.DstMAC, self.SrcMAC = bytes(f["eth_dst"]), bytes(f["eth_src"])
        self.EthernetType, self.Length = int(f["eth_type"]), int(f["eth_length"])
        self.Contents, self.Payload = pkt[s:s + 14], pkt[s + 14:payload_end(_lib.DEC_ETHERNET, pkt, s, e, f)]
        self._poff = 14

    def NextLayerType(self):
        """ethernet.go:111-113"""
        return EthernetTypeLayerType(self.EthernetType)

    def LinkFlow(self):
        return NewFlow(EndpointMAC, self.SrcMAC, self.DstMAC)


# ---- layers/dot1q.go:17-41 ---------------------------------------------------
class Dot1Q(BaseLayer):
    kind = _lib.DEC_DOT1Q

    def __init__(self):
        self.Priority = 0
        self.DropEligible = False
        self.VLANIdentifier = 0
        self.Type = 0

    def LayerType(self):
        return LayerTypeDot1Q

    def CanDecode(self):
        return LayerClass([LayerTypeDot1Q])

    def _hydrate(self, d):
        self.Priority = (d[0] & 0xE0) >> 5
        self.DropEligible = d[0] & 0x10 != 0
        self.VLANIdentifier = _be16(d, 0) & 0x0FFF
        self.Type = _be16(d, 2)
        self.Contents, self.Payload = d[:4], d[4:]
        self._poff = 4

    def _fill(self, pkt, s, e, f):
        tci = int(f["d1q_tci"])
        self.Priority, self.DropEligible, self.VLANIdentifier = tci >> 13, bool(tci >> 12 & 1), tci & 0x0FFF
        self.Type = int(f["d1q_type"])
        self.Contents, self.Payload = pkt[s:s + 4], pkt[s + 4:e]
        self._poff = 4

    def NextLayerType(self):
        """dot1q.go:49-51"""
        return EthernetTypeLayerType(self.Type)


IPv4EvilBit, IPv4DontFragment, IPv4MoreFragments = 1 << 2, 1 << 1, 1 << 0


class IPv4Flag(int):
    """ip4.go:22-40"""

    def String(self):
        names = [n for bit, n in ((IPv4EvilBit, "Evil"), (IPv4DontFragment, "DF"), (IPv4MoreFragments, "MF"))
                 if self & bit]
        return "|".join(names)

    __str__ = String


@dataclass
class IPv4Option:
    OptionType: int = 0
    OptionLength: int = 0
    OptionData: Optional[bytes] = None

    def String(self):  # ip4.go:73-75: "IPv4Option(%v:%v)"
        return "IPv4Option(%d:[%s])" % (self.OptionType, " ".join(str(b) for b in (self.OptionData or b"")))

    __str__ = String


class _Checksummed:
    _csum = None  # (error, ChecksumVerificationResult) set from the device record
    _pseudoheader = None  # tcpipchecksum.pseudoheader (TCP, UDP)

    def SetNetworkLayerForChecksum(self, l):
        """tcpip.go:75-85 (TCP and UDP): the IPv4 or IPv6 layer whose addresses
        the pseudo-header of ComputeChecksum uses."""
        from .gopacket import GoError
        if not hasattr(l, "_pseudoheader_checksum"):
            return GoError("cannot use layer type %s for tcp checksum network layer" % l.LayerType().String())
        self._pseudoheader = l
        return None

    def _compute_checksum(self, header_and_payload, proto):
        """tcpipchecksum.computeChecksum (tcpip.go:44-62): (uint32 sum, error)."""
        from .gopacket import ComputeChecksum, GoError
        if self._pseudoheader is None:
            return 0, GoError("TCP/IP layer 4 checksum cannot be computed without network layer... "
                              "call SetNetworkLayerForChecksum to set which layer to use")
        n = len(header_and_payload)
        csum, err = self._pseudoheader._pseudoheader_checksum()
        if err is not None:
            return 0, err
        csum += proto + (n & 0xFFFF) + (n >> 16)
        return ComputeChecksum(header_and_payload, csum & 0xFFFFFFFF), None

    def VerifyChecksum(self):
        """The device's checksum verification of this layer (see DecodingLayerParser)."""
        if self._csum is None:
            raise RuntimeError("no device checksum result attached to this layer")
        return self._csum


# ---- layers/ip4.go:42-271 ----------------------------------------------------
class IPv4(BaseLayer, _Checksummed):
    kind = _lib.DEC_IPV4

    def __init__(self):
        self.Version = self.IHL = self.TOS = 0
        self.Length = self.Id = 0
        self.Flags = self.FragOffset = 0
        self.TTL = self.Protocol = self.Checksum = 0
        self.SrcIP = self.DstIP = b""
        self.Options: List[IPv4Option] = []
        self.Padding = None

    def LayerType(self):
        return LayerTypeIPv4

    def CanDecode(self):
        return LayerClass([LayerTypeIPv4])

    def _hydrate(self, d):
        self.Length = _be16(d, 2)
        self.IHL = d[0] & 0x0F
        if self.Length == 0:
            self.Length = len(d) & 0xFFFF
        if len(d) > self.Length:
            d = d[:self.Length]
        hl = self.IHL * 4
        self.Options = []
        self.Contents, self.Payload = d[:hl], d[hl:]
        opts = d[20:hl]
        while len(opts) > 0:
            t = opts[0]
            if t == 0:
                self.Options.append(IPv4Option(0, 1))
                self.Padding = opts[1:]
                break
            if t == 1:
                self.Options.append(IPv4Option(1, 1))
                opts = opts[1:]
                continue
            ol = opts[1]
            self.Options.append(IPv4Option(t, ol, opts[2:ol]))
            opts = opts[ol:]
        ff = _be16(d, 6)
        self.Version = d[0] >> 4
        self.TOS = d[1]
        self.Id = _be16(d, 4)
        self.Flags = IPv4Flag(ff >> 13)
        self.FragOffset = ff & 0x1FFF
        self.TTL = d[8]
        self.Protocol = d[9]
        self.Checksum = _be16(d, 10)
        self.SrcIP = d[12:16]
        self.DstIP = d[16:20]
        self._poff = hl

    def _fill(self, pkt, s, e, f):
        self.Version, self.IHL, self.TOS = int(f["ip4_version"]), int(f["ip4_ihl"]), int(f["ip4_tos"])
        self.Length, self.Id = int(f["ip4_length"]), int(f["ip4_id"])
        ff = int(f["ip4_flags_frag"])
        self.Flags, self.FragOffset = IPv4Flag(ff >> 13), ff & 0x1FFF
        self.TTL, self.Protocol, self.Checksum = int(f["ip4_ttl"]), int(f["ip4_protocol"]), int(f["ip4_checksum"])
        self.SrcIP, self.DstIP = bytes(f["ip4_src"]), bytes(f["ip4_dst"])
        hl = self.IHL * 4
        self.Contents, self.Payload = pkt[s:s + hl], pkt[s + hl:payload_end(_lib.DEC_IPV4, pkt, s, e, f)]
        self.Options, padding = IPv4OptionsFromMap(pkt, s, hl, f["ip4_opt_map"])
        if padding is not None:  # set only by an End of options (ip4.go:231), else kept
            self.Padding = padding
        self._poff = hl

    def NextLayerType(self):
        """ip4.go:277-282: a fragment (MoreFragments or an offset) decodes as Fragment"""
        if self.Flags & 1 or self.FragOffset != 0:
            return LayerTypeFragment
        return IPProtocolLayerType(self.Protocol)

    def NetworkFlow(self):
        return NewFlow(EndpointIPv4, self.SrcIP, self.DstIP)

    def AddressTo4(self):
        """ip4.go:295-321: both addresses in their 4-byte form, or the error."""
        from .gopacket import GoError

        def check(a):
            c = _to4(bytes(a))
            if c is not None:
                return c, None
            if len(a) == 16:
                return None, "address is IPv6"
            return None, "wrong length of %d bytes instead of 4" % len(a)

        src, e = check(self.SrcIP)
        if e:
            return GoError("Invalid source IPv4 address (%s)" % e)
        dst, e = check(self.DstIP)
        if e:
            return GoError("Invalid destination IPv4 address (%s)" % e)
        self.SrcIP, self.DstIP = src, dst
        return None

    def _pseudoheader_checksum(self):  # tcpip.go:19-28
        err = self.AddressTo4()
        if err is not None:
            return 0, err
        s_, d_ = self.SrcIP, self.DstIP
        csum = ((s_[0] + s_[2]) << 8) + s_[1] + s_[3] + ((d_[0] + d_[2]) << 8) + d_[1] + d_[3]
        return csum, None


@dataclass
class IPv6HopByHopOption:
    OptionType: int = 0
    OptionLength: int = 0
    ActualLength: int = 0
    OptionData: Optional[bytes] = None


class IPv6HopByHop(BaseLayer):
    def __init__(self):
        self.NextHeader = 0
        self.HeaderLength = 0
        self.ActualLength = 0
        self.Options: List[IPv6HopByHopOption] = []

    def LayerType(self):
        return LayerTypeIPv6HopByHop


# ---- layers/ip6.go:28-278 ----------------------------------------------------
class IPv6(BaseLayer, _Checksummed):
    kind = _lib.DEC_IPV6

    def __init__(self):
        self.Version = self.TrafficClass = self.FlowLabel = 0
        self.Length = self.NextHeader = self.HopLimit = 0
        self.SrcIP = self.DstIP = b""
        self.HopByHop = None
        self.hbh = IPv6HopByHop()

    def LayerType(self):
        return LayerTypeIPv6

    def CanDecode(self):
        return LayerClass([LayerTypeIPv6])

    def _hydrate(self, d):
        self.Version = d[0] >> 4
        self.TrafficClass = (_be16(d, 0) >> 4) & 0xFF
        self.FlowLabel = _be32(d, 0) & 0x000FFFFF
        self.Length = _be16(d, 4)
        self.NextHeader = d[6]
        self.HopLimit = d[7]
        self.SrcIP, self.DstIP = d[8:24], d[24:40]
        self.HopByHop = None
        self.Contents, self.Payload = d[:40], d[40:]
        if self.NextHeader == IPProtocolIPv6HopByHop:
            h, p = self.hbh, self.Payload
            h.NextHeader, h.HeaderLength = p[0], p[1]
            h.ActualLength = p[1] * 8 + 8
            h.Contents, h.Payload = p[:h.ActualLength], p[h.ActualLength:]
            h.Options = []
            off = 2
            while off < h.ActualLength:
                if p[off] == 0:
                    o = IPv6HopByHopOption(0, 0, 1, None)
                else:
                    al = p[off + 1] + 2
                    o = IPv6HopByHopOption(p[off], p[off + 1], al, p[off + 2:off + al])
                h.Options.append(o)
                off += o.ActualLength
            self.HopByHop = h
            jumbo = next((o for o in h.Options if o.OptionType == IPv6HopByHopOptionJumbogram), None)
            if jumbo is not None and self.Length == 0:
                self.Payload = self.Payload[:min(_be32(jumbo.OptionData, 0), len(self.Payload))]
                self._poff = 40
                return
            self.Payload = self.Payload[h.ActualLength:]
        self.Payload = self.Payload[:min(self.Length, len(self.Payload))]
        self._poff = 40 + (self.hbh.ActualLength if self.HopByHop is not None else 0)

    def _fill(self, pkt, s, e, f):
        self.Version, self.TrafficClass = int(f["ip6_version"]), int(f["ip6_traffic_class"])
        self.FlowLabel, self.Length = int(f["ip6_flow_label"]), int(f["ip6_length"])
        self.NextHeader, self.HopLimit = int(f["ip6_next_header"]), int(f["ip6_hop_limit"])
        self.SrcIP, self.DstIP = bytes(f["ip6_src"]), bytes(f["ip6_dst"])
        self.HopByHop = None
        self.Contents = pkt[s:s + 40]
        if self.NextHeader == IPProtocolIPv6HopByHop:
            HopByHopFromMap(self.hbh, pkt, s + 40, e, f["hbh_opt_map"])
            self.HopByHop = self.hbh
        self._poff = ipv6_payload_start(pkt, s, f) - s
        self.Payload = pkt[s + self._poff:payload_end(_lib.DEC_IPV6, pkt, s, e, f)]

    def NextLayerType(self):
        """ip6.go:286-291"""
        if self.HopByHop is not None:
            return IPProtocolLayerType(self.HopByHop.NextHeader)
        return IPProtocolLayerType(self.NextHeader)

    def NetworkFlow(self):
        return NewFlow(EndpointIPv6, self.SrcIP, self.DstIP)

    def AddressTo16(self):
        """ip6.go:742-761: an error unless both addresses are 16 bytes."""
        from .gopacket import GoError
        for which, a in (("source", self.SrcIP), ("destination", self.DstIP)):
            if len(a) != 16:
                e = "address is IPv4" if len(a) == 4 else "wrong length of %d bytes instead of 16" % len(a)
                return GoError("Invalid %s IPv6 address (%s)" % (which, e))
        return None

    def _pseudoheader_checksum(self):  # tcpip.go:30-42
        err = self.AddressTo16()
        if err is not None:
            return 0, err
        csum = 0
        for i in range(0, 16, 2):
            csum += (self.SrcIP[i] << 8) + self.SrcIP[i + 1] + (self.DstIP[i] << 8) + self.DstIP[i + 1]
        return csum & 0xFFFFFFFF, None


def _map_bits(opt_map):
    m = int.from_bytes(bytes(bytearray(opt_map)), "little")
    k = 0
    while m:
        if m & 1:
            yield k
        m >>= 1
        k += 1


def IPv4OptionsFromMap(pkt, start, hlen, opt_map):
    """IPv4.Options and IPv4.Padding (ip4.go:219-256) of the header at
    pkt[start:start+hlen] from its gpk_fields option map (include/gpk.h: bit k
    = an option at header byte 20 + k), reading only the option bytes."""
    opts, padding = [], None
    for k in _map_bits(opt_map):
        b = start + 20 + k
        t = pkt[b]
        if t == 0:
            opts.append(IPv4Option(0, 1))
            padding = pkt[b + 1:start + hlen]
            break
        if t == 1:
            opts.append(IPv4Option(1, 1))
            continue
        ol = pkt[b + 1]
        opts.append(IPv4Option(t, ol, pkt[b + 2:b + ol]))
    return opts, padding


def hbh_map_covers(pkt, hbh_start):
    """Whether a gpk_fields hbh_opt_map holds the HopByHop header at
    pkt[hbh_start]: HeaderLength <= 2 (include/gpk.h)."""
    return pkt[hbh_start + 1] <= 2


def HopByHopFromMap(h, pkt, b0, e, opt_map):
    """IPv6HopByHop (ip6.go:418-432 base, :509-526 options, TLVs :327-346) of
    the header at pkt[b0] inside the IPv6 slice ending at e, from its
    gpk_fields option map: NextHeader and HeaderLength are the header's two
    bytes, each option read at its start."""
    h.NextHeader, h.HeaderLength = pkt[b0], pkt[b0 + 1]
    h.ActualLength = h.HeaderLength * 8 + 8
    h.Contents, h.Payload = pkt[b0:b0 + h.ActualLength], pkt[b0 + h.ActualLength:e]
    h.Options = []
    for k in _map_bits(opt_map):
        b = b0 + 2 + k
        if pkt[b] == 0:  # Pad1
            h.Options.append(IPv6HopByHopOption(0, 0, 1, None))
        else:
            al = pkt[b + 1] + 2
            h.Options.append(IPv6HopByHopOption(pkt[b], pkt[b + 1], al, pkt[b + 2:b + al]))
    return h


def _hbh_jumbo(pkt, b0, opt_map):
    """The jumbogram length of the HopByHop header at pkt[b0] (ip6.go:54-76:
    the first option of type 0xC2), or None."""
    for k in _map_bits(opt_map):
        b = b0 + 2 + k
        if pkt[b] == IPv6HopByHopOptionJumbogram:
            return _be32(pkt, b + 2)
    return None


def ipv6_payload_start(pkt, s, f):
    """Where the IPv6 layer at pkt[s]'s Payload starts (ip6.go:235-262): after
    the 40-byte header, and after an inline HopByHop header unless it is a
    jumbogram (P4: its payload is not advanced past the HopByHop header)."""
    if int(f["ip6_next_header"]) != IPProtocolIPv6HopByHop:
        return s + 40
    if int(f["ip6_length"]) == 0 and _hbh_jumbo(pkt, s + 40, f["hbh_opt_map"]) is not None:
        return s + 40
    return s + 40 + pkt[s + 41] * 8 + 8


def payload_end(kind, pkt, s, e, f):
    """The end of the Payload of the decoder `kind` whose DecodeFromBytes was
    handed pkt[s:e], from its gpk_fields values (each decoder's trim rule)."""
    if kind == _lib.DEC_ETHERNET:  # ethernet.go:50-55: 802.3 length trims, never grows
        return s + 14 + int(f["eth_length"]) if int(f["eth_type"]) == 0 and e - s - 14 > int(f["eth_length"]) else e
    if kind == _lib.DEC_IPV4:  # ip4.go:189-205 (Length already the slice's uint16 length when 0, P9)
        return s + int(f["ip4_length"]) if e - s > int(f["ip4_length"]) else e
    if kind == _lib.DEC_IPV6:  # ip6.go:244-277 (P3 / P4)
        p0, length = ipv6_payload_start(pkt, s, f), int(f["ip6_length"])
        if int(f["ip6_next_header"]) == IPProtocolIPv6HopByHop and length == 0:
            length = _hbh_jumbo(pkt, s + 40, f["hbh_opt_map"])
        return min(e, p0 + length) if p0 <= e else p0
    if kind == _lib.DEC_UDP:  # udp.go:46-55
        ln = int(f["udp_length"])
        return s + min(ln, e - s) if ln >= 8 else e
    return e


# ---- layers/ip6.go:434-461 ---------------------------------------------------
class IPv6ExtensionSkipper(BaseLayer):
    kind = _lib.DEC_IPV6_EXT

    def __init__(self):
        self.NextHeader = 0

    def CanDecode(self):
        return LayerClassIPv6Extension

    def NextLayerType(self):
        """ip6.go:458-461"""
        return IPProtocolLayerType(self.NextHeader)

    def _hydrate(self, d):
        actual = d[1] * 8 + 8
        self.NextHeader = d[0]
        self.Contents, self.Payload = d[:actual], d[actual:]
        self._poff = actual

    def _fill(self, pkt, s, e, f):
        # no record fields: NextHeader and HeaderLength are the header's first two bytes (ip6.go:418-461)
        actual = pkt[s + 1] * 8 + 8
        self.NextHeader = pkt[s]
        self.Contents, self.Payload = pkt[s:s + actual], pkt[s + actual:e]
        self._poff = actual


TCPOptionKindEndList, TCPOptionKindNop, TCPOptionKindMSS, TCPOptionKindTimestamps = 0, 1, 2, 8
TCPOptionKindMultipathTCP = 30
_TCP_OPTION_NAMES = {0: "EndList", 1: "NOP", 2: "MSS", 3: "WindowScale", 4: "SACKPermitted", 5: "SACK", 6: "Echo",
                     7: "EchoReply", 8: "Timestamps", 9: "PartialOrderConnectionPermitted",
                     10: "PartialOrderServiceProfile", 11: "CC", 12: "CCNew", 13: "CCEcho", 14: "AltChecksum",
                     15: "AltChecksumData", 30: "MultipathTCP"}  # tcp.go:62-101


def TCPOptionKindString(k):
    return _TCP_OPTION_NAMES.get(int(k), "Unknown(%d)" % int(k))


# ---- layers/multipathtcp.go: MPTCP option subtypes and their structs -----------
(MPTCPSubtypeMPCAPABLE, MPTCPSubtypeMPJOIN, MPTCPSubtypeDSS, MPTCPSubtypeADDADDR, MPTCPSubtypeREMOVEADDR,
 MPTCPSubtypeMPPRIO, MPTCPSubtypeMPFAIL, MPTCPSubtypeMPFASTCLOSE, MPTCPSubtypeMPTCPRST) = range(9)
_MPTCP_NAMES = ["MP_CAPABLE", "MP_JOIN", "DSS", "ADD_ADDR", "REMOVE_ADDR", "MP_PRIO", "MP_FAIL", "MP_FASTCLOSE",
                "MP_TCPRST"]


def MPTCPSubtypeString(k):
    return _MPTCP_NAMES[k] if 0 <= int(k) < len(_MPTCP_NAMES) else "Unknown(%d)" % int(k)


@dataclass
class MPCapable:
    Version: int = 0
    A: bool = False
    B: bool = False
    C: bool = False
    D: bool = False
    E: bool = False
    F: bool = False
    G: bool = False
    H: bool = False
    SendKey: Optional[bytes] = None
    ReceivKey: Optional[bytes] = None
    DataLength: int = 0
    Checksum: int = 0


@dataclass
class MPJoin:
    Backup: bool = False
    AddrID: int = 0
    ReceivToken: int = 0
    SendRandNum: int = 0
    SendHMAC: Optional[bytes] = None


@dataclass
class Dss:
    F: bool = False
    m: bool = False
    M: bool = False
    a: bool = False
    A: bool = False
    DataAck: Optional[bytes] = None
    DSN: Optional[bytes] = None
    SSN: int = 0
    DataLength: int = 0
    Checksum: int = 0


@dataclass
class AddAddr:
    IPVer: int = 0
    E: bool = False
    AddrID: int = 0
    Address: Optional[bytes] = None
    Port: int = 0
    SendHMAC: Optional[bytes] = None


@dataclass
class RemAddr:
    AddrIDs: Optional[list] = None


@dataclass
class MPPrio:
    Backup: bool = False
    AddrID: int = 0


@dataclass
class MPFail:
    DSN: int = 0


@dataclass
class MPFClose:
    ReceivKey: Optional[bytes] = None


@dataclass
class MPTcpRst:
    U: bool = False
    V: bool = False
    W: bool = False
    T: bool = False
    Reason: int = 0


@dataclass
class TCPOption:
    """tcp.go:103-117"""
    OptionType: int = 0
    OptionLength: int = 0
    OptionData: Optional[bytes] = None
    OptionMultipath: int = 0
    OptionMPTCPMpCapable: Optional[MPCapable] = None
    OptionMPTCPDss: Optional[Dss] = None
    OptionMPTCPMpJoin: Optional[MPJoin] = None
    OptionMPTCPMpPrio: Optional[MPPrio] = None
    OptionMPTCPAddAddr: Optional[AddAddr] = None
    OptionMTCPRemAddr: Optional[RemAddr] = None
    OptionMTCPMPFastClose: Optional[MPFClose] = None
    OptionMPTCPMPTcpRst: Optional[MPTcpRst] = None
    OptionMTCPMPFail: Optional[MPFail] = None

    def String(self):
        """tcp.go:120-184"""
        d = self.OptionData or b""
        hd = (" 0x" + d.hex()) if d else ""
        k = TCPOptionKindString(self.OptionType)
        if self.OptionType == TCPOptionKindMSS and len(d) >= 2:
            return "TCPOption(%s:%d%s)" % (k, _be16(d, 0), hd)
        if self.OptionType == TCPOptionKindTimestamps and len(d) == 8:
            return "TCPOption(%s:%d/%d%s)" % (k, _be32(d, 0), _be32(d, 4), hd)
        if self.OptionType == TCPOptionKindMultipathTCP:
            st, n, gb = self.OptionMultipath, MPTCPSubtypeString(self.OptionMultipath), lambda b: str(b).lower()
            if st == MPTCPSubtypeMPCAPABLE:
                return "MPTCPOption(%s Version %d)" % (n, self.OptionMPTCPMpCapable.Version)
            if st == MPTCPSubtypeMPJOIN:
                j = self.OptionMPTCPMpJoin
                return "MPTCPOption(%s Backup %s;Address ID %d)" % (n, gb(j.Backup), j.AddrID)
            if st in (MPTCPSubtypeDSS, MPTCPSubtypeMPFASTCLOSE, MPTCPSubtypeMPFAIL):
                return "MPTCPOption(%s)" % n
            if st == MPTCPSubtypeMPPRIO:
                q = self.OptionMPTCPMpPrio
                return "MPTCPOption(%s Backup %s;Address ID %d)" % (n, gb(q.Backup), q.AddrID)
            if st == MPTCPSubtypeADDADDR:
                a = self.OptionMPTCPAddAddr
                from .gopacket import _ip_string
                return "MPTCPOption(%s Address ID %d;Address %s;Port %d)" % (n, a.AddrID, _ip_string(a.Address or b""),
                                                                           a.Port)
            if st == MPTCPSubtypeREMOVEADDR:
                return "MPTCPOption(%s Address ID [%s])" % (n, " ".join(str(x) for x in self.OptionMTCPRemAddr.AddrIDs))
            if st == MPTCPSubtypeMPTCPRST:
                r = self.OptionMPTCPMPTcpRst
                return "MPTCPOption(%s Transient %s; Reason %d)" % (n, gb(r.T), r.Reason)
        return "TCPOption(%s:%s)" % (k, hd)

    __str__ = String


def _mptcp_option(o, d):
    """The MPTCP option struct tcp.go:346-527 builds from the option at d[0]
    (d: the rest of the options area; the packet decoded without error, so its
    lengths are ones the reference accepts)."""
    L, st = o.OptionLength, o.OptionMultipath
    b16 = lambda a: _be16(d, a)  # noqa: E731
    b32 = lambda a: _be32(d, a)  # noqa: E731
    if st == MPTCPSubtypeMPCAPABLE:
        f = d[3]
        c = MPCapable(d[2] & 0x0F, *(bool(f & (0x80 >> i)) for i in range(8)))
        if L >= 12:
            c.SendKey = bytes(d[4:12])
        if L >= 20:
            c.ReceivKey = bytes(d[12:20])
        if L >= 22:
            c.DataLength = b16(20)
        if L == 24:
            c.Checksum = b16(22)
        o.OptionMPTCPMpCapable = c
    elif st == MPTCPSubtypeMPJOIN:
        if L == 12:
            o.OptionMPTCPMpJoin = MPJoin(bool(d[2] & 1), d[3], b32(4), b32(8))
        elif L == 16:
            o.OptionMPTCPMpJoin = MPJoin(bool(d[2] & 1), d[3], SendHMAC=bytes(d[4:12]), SendRandNum=b32(12))
        elif L == 24:
            o.OptionMPTCPMpJoin = MPJoin(SendHMAC=bytes(d[4:24]))
    elif st == MPTCPSubtypeDSS:
        f = d[3]
        x = Dss(bool(f & 0x10), bool(f & 0x08), bool(f & 0x04), bool(f & 0x02), bool(f & 0x01))
        k = 4
        if x.A:
            n = 8 if x.a else 4
            x.DataAck, k = bytes(d[k:k + n]), k + n
        if x.M:
            n = 8 if x.m else 4
            x.DSN, k = bytes(d[k:k + n]), k + n
            x.SSN, k = b32(k), k + 4
            x.DataLength, k = b16(k), k + 2
            if (L - k) & 0xFF == 2:
                x.Checksum = b16(k)
        o.OptionMPTCPDss = x
    elif st == MPTCPSubtypeADDADDR:
        n = L
        if d[2] & 0x0F > 1:
            a = AddAddr(IPVer=d[2] & 0x0F, AddrID=d[3])
        else:
            a = AddAddr(E=bool(d[2] & 1), AddrID=d[3])
            if not a.E:
                a.SendHMAC = bytes(d[L - 8:])  # to the end of the options area, as Go's data[L-8:]
                n = (n - 8) & 0xFF
        if n in (8, 10):
            a.Address = bytes(d[4:8])
        elif n in (20, 22):
            a.Address = bytes(d[4:20])
        if n == 10:
            a.Port = b16(8)
        elif n == 22:
            a.Port = b16(20)
        o.OptionMPTCPAddAddr = a
    elif st == MPTCPSubtypeREMOVEADDR:
        o.OptionMTCPRemAddr = RemAddr(list(d[3:3 + (L - 3)]))
    elif st == MPTCPSubtypeMPPRIO:
        o.OptionMPTCPMpPrio = MPPrio(bool(d[2] & 1), d[3] if L == 4 else 0)
    elif st == MPTCPSubtypeMPFAIL:
        o.OptionMTCPMPFail = MPFail(struct.unpack(">Q", bytes(d[4:12]))[0])
    elif st == MPTCPSubtypeMPFASTCLOSE:
        o.OptionMTCPMPFastClose = MPFClose(bytes(d[4:12]))
    elif st == MPTCPSubtypeMPTCPRST:
        o.OptionMPTCPMPTcpRst = MPTcpRst(bool(d[2] & 8), bool(d[2] & 4), bool(d[2] & 2), bool(d[2] & 1), d[3])
    return o


# ---- layers/tcp.go:19-551 ----------------------------------------------------
class TCP(BaseLayer, _Checksummed):
    kind = _lib.DEC_TCP

    def __init__(self):
        self.SrcPort = self.DstPort = 0
        self.Seq = self.Ack = 0
        self.DataOffset = 0
        self.FIN = self.SYN = self.RST = self.PSH = self.ACK = self.URG = self.ECE = self.CWR = self.NS = False
        self.Window = self.Checksum = self.Urgent = 0
        self.Options: List[TCPOption] = []
        self.Padding = b""
        self.Multipath = False
        self.sPort = self.dPort = b""

    def LayerType(self):
        return LayerTypeTCP

    def CanDecode(self):
        return LayerClass([LayerTypeTCP])

    def _hydrate(self, d):
        self.SrcPort, self.DstPort = _be16(d, 0), _be16(d, 2)
        self.sPort, self.dPort = d[0:2], d[2:4]
        self.Seq, self.Ack = _be32(d, 4), _be32(d, 8)
        self.DataOffset = d[12] >> 4
        f = d[13]
        self.FIN, self.SYN, self.RST, self.PSH = bool(f & 1), bool(f & 2), bool(f & 4), bool(f & 8)
        self.ACK, self.URG, self.ECE, self.CWR = bool(f & 0x10), bool(f & 0x20), bool(f & 0x40), bool(f & 0x80)
        self.NS = bool(d[12] & 1)
        self.Window, self.Checksum, self.Urgent = _be16(d, 14), _be16(d, 16), _be16(d, 18)
        ds = self.DataOffset * 4
        self.Contents, self.Payload = d[:ds], d[ds:]
        self.Options, self.Padding = [], b""
        opts = d[20:ds]
        while len(opts) > 0:
            t = opts[0]
            if t == 0:
                self.Options.append(TCPOption(0, 1))
                self.Padding = opts[1:]
                break
            if t == 1:
                o = TCPOption(1, 1)
            elif t == TCPOptionKindMultipathTCP:
                self.Multipath = True
                o = _mptcp_option(TCPOption(t, opts[1], None, opts[2] >> 4), opts)
            else:
                o = TCPOption(t, opts[1], opts[2:opts[1]])
            self.Options.append(o)
            opts = opts[o.OptionLength:]
        self._poff = ds

    def _fill(self, pkt, s, e, f):
        self.SrcPort, self.DstPort = int(f["tcp_src_port"]), int(f["tcp_dst_port"])
        self.sPort, self.dPort = struct.pack(">H", self.SrcPort), struct.pack(">H", self.DstPort)
        self.Seq, self.Ack, self.DataOffset = int(f["tcp_seq"]), int(f["tcp_ack"]), int(f["tcp_data_offset"])
        fl = int(f["tcp_flags"])
        self.FIN, self.SYN, self.RST, self.PSH = bool(fl & 1), bool(fl & 2), bool(fl & 4), bool(fl & 8)
        self.ACK, self.URG, self.ECE, self.CWR = bool(fl & 0x10), bool(fl & 0x20), bool(fl & 0x40), bool(fl & 0x80)
        self.NS = bool(fl & 0x100)
        self.Window, self.Checksum, self.Urgent = int(f["tcp_window"]), int(f["tcp_checksum"]), int(f["tcp_urgent"])
        ds = self.DataOffset * 4
        self.Contents, self.Payload = pkt[s:s + ds], pkt[s + ds:e]
        self.Options, self.Padding, mp = TCPOptionsFromMap(pkt, s, ds, f["tcp_opt_map"])
        if mp:  # tcp.go:348: set by an MPTCP option, never reset (P6)
            self.Multipath = True
        self._poff = ds

    def NextLayerType(self):
        """tcp.go:591-597: the destination port's type, else the source port's"""
        lt = TCPPortLayerType(self.DstPort)
        return TCPPortLayerType(self.SrcPort) if lt == LayerTypePayload else lt

    def TransportFlow(self):
        return NewFlow(EndpointTCPPort, self.sPort, self.dPort)

    def ComputeChecksum(self):
        """tcp.go:251-257: (uint16, error) over Contents + Payload as they are
        (the header's own Checksum field included: 0 for a correct segment)."""
        from .gopacket import FoldChecksum
        csum, err = self._compute_checksum(bytes(self.Contents) + bytes(self.Payload), 6)
        return (0, err) if err is not None else (FoldChecksum(csum), None)


def TCPOptionsFromMap(pkt, start, hlen, opt_map):
    """TCP.Options, TCP.Padding and TCP.Multipath (tcp.go:336-549) of the
    header at pkt[start:start+hlen] from its gpk_fields option map."""
    opts, padding, mp = [], b"", False
    for k in _map_bits(opt_map):
        b = start + 20 + k
        t = pkt[b]
        if t == 0:
            opts.append(TCPOption(0, 1))
            padding = pkt[b + 1:start + hlen]
            break
        if t == 1:
            opts.append(TCPOption(1, 1))
        elif t == TCPOptionKindMultipathTCP:
            mp = True
            opts.append(_mptcp_option(TCPOption(t, pkt[b + 1], None, pkt[b + 2] >> 4), pkt[b:start + hlen]))
        else:
            opts.append(TCPOption(t, pkt[b + 1], pkt[b + 2:b + pkt[b + 1]]))
    return opts, padding, mp


# ---- layers/udp.go:17-56 -----------------------------------------------------
class UDP(BaseLayer, _Checksummed):
    kind = _lib.DEC_UDP

    def __init__(self):
        self.SrcPort = self.DstPort = self.Length = self.Checksum = 0
        self.sPort = self.dPort = b""

    def LayerType(self):
        return LayerTypeUDP

    def CanDecode(self):
        return LayerClass([LayerTypeUDP])

    def _hydrate(self, d):
        self.SrcPort, self.DstPort = _be16(d, 0), _be16(d, 2)
        self.sPort, self.dPort = d[0:2], d[2:4]
        self.Length, self.Checksum = _be16(d, 4), _be16(d, 6)
        self.Contents = d[:8]
        if self.Length >= 8:
            self.Payload = d[8:min(self.Length, len(d))]
        else:
            self.Payload = d[8:]
        self._poff = 8

    def _fill(self, pkt, s, e, f):
        self.SrcPort, self.DstPort = int(f["udp_src_port"]), int(f["udp_dst_port"])
        self.sPort, self.dPort = struct.pack(">H", self.SrcPort), struct.pack(">H", self.DstPort)
        self.Length, self.Checksum = int(f["udp_length"]), int(f["udp_checksum"])
        self.Contents, self.Payload = pkt[s:s + 8], pkt[s + 8:payload_end(_lib.DEC_UDP, pkt, s, e, f)]
        self._poff = 8

    def NextLayerType(self):
        """udp.go:114-119"""
        lt = UDPPortLayerType(self.DstPort)
        return lt if lt != LayerTypePayload else UDPPortLayerType(self.SrcPort)

    def TransportFlow(self):
        return NewFlow(EndpointUDPPort, self.sPort, self.dPort)


__all__ = [n for n in dir() if not n.startswith("_")]


# ---- endpoints (layers/endpoints.go:51-99) --------------------------------------


def _to4(ip):  # net.IP.To4
    if len(ip) == 4:
        return ip
    if len(ip) == 16 and ip[:10] == bytes(10) and ip[10:12] == b"\xff\xff":
        return ip[12:]
    return None


def NewIPEndpoint(ip):
    """An IPv4 endpoint for a 4-byte or IPv4-mapped address, IPv6 for another
    16-byte one, InvalidEndpoint otherwise (ip: bytes or an ipaddress object)."""
    b = ip.packed if hasattr(ip, "packed") else bytes(ip)
    v4 = _to4(b)
    if v4 is not None:
        return NewEndpoint(EndpointIPv4, v4)
    if len(b) == 16:
        return NewEndpoint(EndpointIPv6, b)
    return InvalidEndpoint


def NewMACEndpoint(mac):
    return NewEndpoint(EndpointMAC, bytes(mac))


def _port_endpoint(t, p):
    return NewEndpoint(t, bytes([(p >> 8) & 0xFF, p & 0xFF]))


def NewTCPPortEndpoint(p):
    return _port_endpoint(EndpointTCPPort, int(p))


def NewUDPPortEndpoint(p):
    return _port_endpoint(EndpointUDPPort, int(p))


def NewSCTPPortEndpoint(p):
    return _port_endpoint(EndpointSCTPPort, int(p))


def NewRUDPPortEndpoint(p):
    return NewEndpoint(EndpointRUDPPort, bytes([int(p) & 0xFF]))


def NewUDPLitePortEndpoint(p):
    return _port_endpoint(EndpointUDPLitePort, int(p))


# ---- tunnel layers: layers/gre.go, vxlan.go, geneve.go --------------------------
# A DecodingLayerParser that holds one of these peels tunnel levels on the
# device (gpk_tunnel_batch); the structs are filled from the level's gpk_tunnel
# record and the packet bytes of that level (_from_record). `kind` values
# above the device decoders' keep them apart in a container.
class _TunnelLayer(BaseLayer):
    def DecodeFromBytes(self, data, df):
        raise NotImplementedError("tunnel layers decode through a DecodingLayerParser (DecodeLayers / DecodeBatch)")


@dataclass
class GRERouting:
    """gre.go:27-34"""
    AddressFamily: int = 0
    SREOffset: int = 0
    SRELength: int = 0
    RoutingInformation: bytes = b""
    Next: Optional["GRERouting"] = None


class GRE(_TunnelLayer):
    kind = 100 + _lib.TUN_GRE
    tunnel_kind = _lib.TUN_GRE

    def __init__(self):
        self.ChecksumPresent = self.RoutingPresent = self.KeyPresent = self.SeqPresent = False
        self.StrictSourceRoute = self.AckPresent = False
        self.RecursionControl = self.Flags = self.Version = 0
        self.Protocol = 0
        self.Checksum = self.Offset = 0
        self.Key = self.Seq = self.Ack = 0
        self.GRERouting = None
        self._csum = None

    def LayerType(self):
        return LayerTypeGRE

    def CanDecode(self):
        return LayerClass([LayerTypeGRE])

    def NextLayerType(self):
        """gre.go:235-237"""
        return EthernetTypeLayerType(self.Protocol)

    def _from_record(self, t, pkt):
        b0, b1 = int(t["raw0"]), int(t["raw1"])
        self.ChecksumPresent, self.RoutingPresent = bool(b0 & 0x80), bool(b0 & 0x40)
        self.KeyPresent, self.SeqPresent, self.StrictSourceRoute = bool(b0 & 0x20), bool(b0 & 0x10), bool(b0 & 0x08)
        self.AckPresent = bool(b1 & 0x80)
        self.RecursionControl, self.Flags, self.Version = b0 & 7, b1 >> 3, b1 & 7
        self.Protocol = int(t["protocol"])
        self.Checksum, self.Offset = int(t["gre_checksum"]), int(t["gre_offset"])
        self.Key, self.Seq, self.Ack = int(t["gre_key"]), int(t["gre_seq"]), int(t["gre_ack"])
        h, c = int(t["hdr_off"]), int(t["contents_len"])
        self.Contents, self.Payload = pkt[h:h + c], pkt[h + c:h + c + int(t["inner_len"])]
        self.GRERouting = None
        o, sres = int(t["list_off"]), []
        for _ in range(int(t["count"])):
            sl = pkt[o + 3]
            sres.append(GRERouting(_be16(pkt, o), pkt[o + 2], sl, pkt[o + 4:o + 4 + sl]))
            o += 4 + sl
        for sre in reversed(sres):
            sre.Next, self.GRERouting = self.GRERouting, sre
        st = int(t["status"])
        self._csum = None
        if st & _lib.TUN_ST_CSUM:
            self._csum = (None, ChecksumVerificationResult(bool(st & _lib.TUN_ST_VALID), int(t["gre_correct"]),
                                                           self.Checksum))

    def VerifyChecksum(self):
        """gre.go:239-250; the device's sum when the header has the C bit and
        the level was peeled with gre_checksum, else computed here."""
        if self._csum is not None:
            return self._csum
        from .gopacket import ComputeChecksum, FoldChecksum
        correct = FoldChecksum((ComputeChecksum(self.Contents + self.Payload, 0) - self.Checksum) & 0xFFFFFFFF)
        return None, ChecksumVerificationResult(not self.ChecksumPresent or correct == self.Checksum, correct,
                                                self.Checksum)


class VXLAN(_TunnelLayer):
    kind = 100 + _lib.TUN_VXLAN
    tunnel_kind = _lib.TUN_VXLAN

    def __init__(self):
        self.ValidIDFlag = self.GBPExtension = self.GBPDontLearn = self.GBPApplied = False
        self.VNI = 0
        self.GBPGroupPolicyID = 0

    def LayerType(self):
        return LayerTypeVXLAN

    def CanDecode(self):
        return LayerClass([LayerTypeVXLAN])

    def NextLayerType(self):
        """vxlan.go:48-50"""
        return LayerTypeEthernet

    def _from_record(self, t, pkt):
        bits = int(t["bits"])
        self.ValidIDFlag, self.GBPExtension = bool(bits & _lib.TUN_VX_I), bool(bits & _lib.TUN_VX_G)
        self.GBPDontLearn, self.GBPApplied = bool(bits & _lib.TUN_VX_D), bool(bits & _lib.TUN_VX_A)
        self.VNI, self.GBPGroupPolicyID = int(t["vni"]), int(t["gbp_id"])
        h, c = int(t["hdr_off"]), int(t["contents_len"])
        self.Contents, self.Payload = pkt[h:h + c], pkt[h + c:h + c + int(t["inner_len"])]


@dataclass
class GeneveOption:
    """geneve.go:45-51"""
    Class: int = 0
    Type: int = 0
    Flags: int = 0
    Length: int = 0
    Data: bytes = b""


class Geneve(_TunnelLayer):
    kind = 100 + _lib.TUN_GENEVE
    tunnel_kind = _lib.TUN_GENEVE

    def __init__(self):
        self.Version = self.OptionsLength = 0
        self.OAMPacket = self.CriticalOption = False
        self.Protocol = 0
        self.VNI = 0
        self.Options = []

    def LayerType(self):
        return LayerTypeGeneve

    def CanDecode(self):
        return LayerClass([LayerTypeGeneve])

    def NextLayerType(self):
        """geneve.go:121-123"""
        return EthernetTypeLayerType(self.Protocol)

    def _from_record(self, t, pkt):
        bits = int(t["bits"])
        self.Version, self.OptionsLength = int(t["gn_version"]), int(t["gn_options_length"])
        self.OAMPacket, self.CriticalOption = bool(bits & _lib.TUN_GN_O), bool(bits & _lib.TUN_GN_C)
        self.Protocol, self.VNI = int(t["protocol"]), int(t["vni"])
        h, c = int(t["hdr_off"]), int(t["contents_len"])
        self.Contents, self.Payload = pkt[h:h + c], pkt[h + c:h + c + int(t["inner_len"])]
        # the reference's walk (geneve.go:105-114): the offset is a uint8 and wraps
        self.Options, o = [], 8
        for _ in range(int(t["count"])):
            b3 = pkt[h + o + 3]
            ln = (b3 & 0x1f) * 4 + 4
            self.Options.append(GeneveOption(_be16(pkt, h + o), pkt[h + o + 2], b3 >> 5, ln, pkt[h + o + 4:h + o + ln]))
            o = (o + ln) & 0xff


# ---- control layers: layers/icmp4.go, icmp6.go, icmp6msg.go, arp.go ---------------
# A DecodingLayerParser that holds one of these decodes them on the device
# after the six-layer decode (gpk_control_batch); the structs are filled from
# the packet's gpk_control record and its bytes (_from_record).
class _ControlLayer(BaseLayer):
    def DecodeFromBytes(self, data, df):
        raise NotImplementedError("control layers decode through a DecodingLayerParser (DecodeLayers / DecodeBatch)")


class _TypeCode(int):
    """icmp4.go:51-62 / icmp6.go:62-73: the type in the high byte, the code in the low one."""

    def Type(self):
        return int(self) >> 8

    def Code(self):
        return int(self) & 0xFF


class ICMPv4TypeCode(_TypeCode):
    pass


class ICMPv6TypeCode(_TypeCode):
    pass


def CreateICMPv4TypeCode(typ, code):
    return ICMPv4TypeCode((typ & 0xFF) << 8 | (code & 0xFF))


def CreateICMPv6TypeCode(typ, code):
    return ICMPv6TypeCode((typ & 0xFF) << 8 | (code & 0xFF))


def _control_checksum(t, checksum):
    """The (err, ChecksumVerificationResult) of a gpk_control record, or None when no sum was asked for."""
    from .gopacket import GoError
    st = int(t["status"])
    if st & _lib.CTL_ST_CSUM:
        return (None, ChecksumVerificationResult(bool(st & _lib.CTL_ST_VALID), int(t["correct"]), checksum))
    if st & _lib.CTL_ST_NONET:  # tcpip.go:55-57
        return (GoError("TCP/IP layer 4 checksum cannot be computed without network layer... call "
                        "SetNetworkLayerForChecksum to set which layer to use"), ChecksumVerificationResult())
    return None


class ICMPv4(_ControlLayer):
    """icmp4.go:209-276"""
    kind = 200 + _lib.CTL_ICMP4
    control_kind = _lib.CTL_ICMP4

    def __init__(self):
        self.TypeCode = ICMPv4TypeCode(0)
        self.Checksum = self.Id = self.Seq = 0
        self._csum = None

    def LayerType(self):
        return LayerTypeICMPv4

    def CanDecode(self):
        return LayerClass([LayerTypeICMPv4])

    def NextLayerType(self):
        return LayerTypePayload

    def _from_record(self, t, pkt):
        self.TypeCode = ICMPv4TypeCode(int(t["typecode"]))
        self.Checksum, self.Id, self.Seq = int(t["checksum"]), int(t["id"]), int(t["seq"])
        h, c = int(t["hdr_off"]), int(t["contents_len"])
        self.Contents, self.Payload = pkt[h:h + c], pkt[h + c:h + c + int(t["payload_len"])]
        self._csum = _control_checksum(t, self.Checksum)

    def VerifyChecksum(self):
        """icmp4.go:265-276: the device's sum when the batch was decoded with checksum=True, else computed here."""
        if self._csum is not None:
            return self._csum
        from .gopacket import ComputeChecksum, FoldChecksum
        correct = FoldChecksum((ComputeChecksum(self.Contents + self.Payload, 0) - self.Checksum) & 0xFFFFFFFF)
        return None, ChecksumVerificationResult(correct == self.Checksum, correct, self.Checksum)


class ICMPv6(_ControlLayer):
    """icmp6.go:170-277"""
    kind = 200 + _lib.CTL_ICMP6
    control_kind = _lib.CTL_ICMP6

    def __init__(self):
        self.TypeCode = ICMPv6TypeCode(0)
        self.Checksum = 0
        self._next = LayerTypePayload
        self._csum = None

    def LayerType(self):
        return LayerTypeICMPv6

    def CanDecode(self):
        return LayerClass([LayerTypeICMPv6])

    def NextLayerType(self):
        """icmp6.go:230-261 (worked out on the device: gpk_control.next_type)"""
        return self._next

    def _from_record(self, t, pkt):
        self.TypeCode = ICMPv6TypeCode(int(t["typecode"]))
        self.Checksum = int(t["checksum"])
        h, c = int(t["hdr_off"]), int(t["contents_len"])
        self.Contents, self.Payload = pkt[h:h + c], pkt[h + c:h + c + int(t["payload_len"])]
        self._next = LayerType(int(t["next_type"]))
        self._csum = _control_checksum(t, self.Checksum)

    def VerifyChecksum(self):
        """icmp6.go:263-277 with the pseudo-header of the last network layer of
        the decoded list (the device's sum). A batch decoded with
        checksum=False has none: the reference's error for a layer without
        SetNetworkLayerForChecksum."""
        if self._csum is not None:
            return self._csum
        from .gopacket import GoError
        return (GoError("TCP/IP layer 4 checksum cannot be computed without network layer... call "
                        "SetNetworkLayerForChecksum to set which layer to use"), ChecksumVerificationResult())


class ICMPv6Echo(_ControlLayer):
    """icmp6msg.go:122-164. DecodeFromBytes sets no BaseLayer: Contents and Payload stay empty."""
    kind = 200 + _lib.CTL_ICMP6ECHO
    control_kind = _lib.CTL_ICMP6ECHO

    def __init__(self):
        self.Identifier = self.SeqNumber = 0

    def LayerType(self):
        return LayerTypeICMPv6Echo

    def CanDecode(self):
        return LayerClass([LayerTypeICMPv6Echo])

    def NextLayerType(self):
        return LayerTypePayload

    def _from_record(self, t, pkt):
        self.Identifier, self.SeqNumber = int(t["id"]), int(t["seq"])
        self.Contents = self.Payload = b""


class ARP(_ControlLayer):
    """arp.go:25-108"""
    kind = 200 + _lib.CTL_ARP
    control_kind = _lib.CTL_ARP

    def __init__(self):
        self.AddrType = self.Protocol = self.HwAddressSize = self.ProtAddressSize = self.Operation = 0
        self.SourceHwAddress = self.SourceProtAddress = self.DstHwAddress = self.DstProtAddress = b""

    def LayerType(self):
        return LayerTypeARP

    def CanDecode(self):
        return LayerClass([LayerTypeARP])

    def NextLayerType(self):
        return LayerTypePayload

    def _from_record(self, t, pkt):
        self.AddrType, self.Protocol = int(t["arp_addr_type"]), int(t["arp_protocol"])
        self.HwAddressSize, self.ProtAddressSize = int(t["arp_hw_size"]), int(t["arp_prot_size"])
        self.Operation = int(t["arp_operation"])
        h, c, hw, pr = int(t["hdr_off"]), int(t["contents_len"]), self.HwAddressSize, self.ProtAddressSize
        a = h + 8
        self.SourceHwAddress, self.SourceProtAddress = pkt[a:a + hw], pkt[a + hw:a + hw + pr]
        self.DstHwAddress, self.DstProtAddress = pkt[a + hw + pr:a + 2 * hw + pr], pkt[a + 2 * hw + pr:h + c]
        self.Contents, self.Payload = pkt[h:h + c], pkt[h + c:h + c + int(t["payload_len"])]


# ---- layers/icmp6msg.go, mldv1.go, mldv2.go: the messages behind ICMPv6 ---------------
# A DecodingLayerParser that holds one of these decodes them on the device after
# the control pass (gpk_ndp_batch); the structs are filled from the packet's
# gpk_ndp record, its gpk_ndp_entry descriptors and the packet's bytes
# (_from_record). Every message is decoded into a fresh struct: the lists are
# the message's own (include/gpk_ndp.h, Scope decisions). A time.Duration is an
# int of nanoseconds.
_SECOND, _MILLISECOND = 1000000000, 1000000


class ICMPv6Opt(int):
    """icmp6msg.go:24-60, 120-137"""

    def String(self):
        return _ICMPV6_OPT_NAMES.get(int(self), "Unknown(%d)" % int(self))


(ICMPv6OptSourceAddress, ICMPv6OptTargetAddress, ICMPv6OptPrefixInfo, ICMPv6OptRedirectedHeader, ICMPv6OptMTU) = (
    ICMPv6Opt(k) for k in range(1, 6))
ICMPv6OptRecursiveDNSServer = ICMPv6Opt(25)
_ICMPV6_OPT_NAMES = {1: "SourceAddress", 2: "TargetAddress", 3: "PrefixInfo", 4: "RedirectedHeader", 5: "MTU",
                     25: "RecursiveDNSServer"}


class ICMPv6Option:
    """icmp6msg.go:111-115"""

    def __init__(self, Type=0, Data=b""):
        self.Type, self.Data = ICMPv6Opt(Type), bytes(Data)

    def __eq__(self, o):
        return isinstance(o, ICMPv6Option) and (int(self.Type), self.Data) == (int(o.Type), o.Data)

    def __repr__(self):
        return "ICMPv6Option(%s, %r)" % (self.Type.String(), self.Data)


class ICMPv6Options(list):
    """icmp6msg.go:118"""


class _NDPLayer(BaseLayer):
    _lt = None

    def DecodeFromBytes(self, data, df):
        raise NotImplementedError("NDP and MLD layers decode through a DecodingLayerParser (DecodeLayers / DecodeBatch)")

    def LayerType(self):
        return self._lt

    def CanDecode(self):
        return LayerClass([self._lt])

    def NextLayerType(self):
        return LayerTypePayload

    def _base(self, t, pkt):
        """BaseLayer from the record's ranges; the options of the entries."""
        h = int(t["hdr_off"])
        self.Contents = pkt[h:h + int(t["contents_len"])]
        o = int(t["payload_off"])
        self.Payload = pkt[o:o + int(t["payload_len"])]

    @staticmethod
    def _options(entries, pkt):
        return ICMPv6Options(ICMPv6Option(int(e["type"]), pkt[int(e["off"]):int(e["off"]) + int(e["ext"])])
                             for e in entries)

    @staticmethod
    def _ip(t, k, pkt):
        return pkt[int(t["v"][k]):int(t["v"][k]) + 16]


class ICMPv6RouterSolicitation(_NDPLayer):
    """icmp6msg.go:69-73, 180-224. DecodeFromBytes sets no BaseLayer."""
    kind = 400 + 0
    ndp_kind = _lib.NDP_RS
    _lt = LayerTypeICMPv6RouterSolicitation

    def __init__(self):
        self.Options = ICMPv6Options()

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        self.Options = self._options(entries, pkt)


class ICMPv6RouterAdvertisement(_NDPLayer):
    """icmp6msg.go:75-84, 226-293"""
    kind = 400 + 1
    ndp_kind = _lib.NDP_RA
    _lt = LayerTypeICMPv6RouterAdvertisement

    def __init__(self):
        self.HopLimit = self.Flags = self.RouterLifetime = self.ReachableTime = self.RetransTimer = 0
        self.Options = ICMPv6Options()

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        v = t["v"]
        self.ReachableTime, self.RetransTimer, self.RouterLifetime, self.HopLimit = (int(x) for x in v)
        self.Flags = int(t["flags"])
        self.Options = self._options(entries, pkt)

    def ManagedAddressConfig(self):
        return self.Flags & 0x80 != 0

    def OtherConfig(self):
        return self.Flags & 0x40 != 0


class ICMPv6NeighborSolicitation(_NDPLayer):
    """icmp6msg.go:86-92, 295-342"""
    kind = 400 + 2
    ndp_kind = _lib.NDP_NS
    _lt = LayerTypeICMPv6NeighborSolicitation

    def __init__(self):
        self.TargetAddress = b""
        self.Options = ICMPv6Options()

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        self.TargetAddress = self._ip(t, 0, pkt)
        self.Options = self._options(entries, pkt)


class ICMPv6NeighborAdvertisement(_NDPLayer):
    """icmp6msg.go:94-100, 344-409"""
    kind = 400 + 3
    ndp_kind = _lib.NDP_NA
    _lt = LayerTypeICMPv6NeighborAdvertisement

    def __init__(self):
        self.Flags = 0
        self.TargetAddress = b""
        self.Options = ICMPv6Options()

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        self.Flags = int(t["flags"])
        self.TargetAddress = self._ip(t, 0, pkt)
        self.Options = self._options(entries, pkt)

    def Router(self):
        return self.Flags & 0x80 != 0

    def Solicited(self):
        return self.Flags & 0x40 != 0

    def Override(self):
        return self.Flags & 0x20 != 0


class ICMPv6Redirect(_NDPLayer):
    """icmp6msg.go:102-109, 411-460"""
    kind = 400 + 4
    ndp_kind = _lib.NDP_REDIRECT
    _lt = LayerTypeICMPv6Redirect

    def __init__(self):
        self.TargetAddress = self.DestinationAddress = b""
        self.Options = ICMPv6Options()

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        self.TargetAddress, self.DestinationAddress = self._ip(t, 0, pkt), self._ip(t, 1, pkt)
        self.Options = self._options(entries, pkt)


class MLDv1Message(_NDPLayer):
    """mldv1.go:20-48. DecodeFromBytes sets no BaseLayer; NextLayerType is LayerTypeZero."""

    def __init__(self):
        self.MaximumResponseDelay = 0  # time.Duration: nanoseconds
        self.MulticastAddress = b""

    def NextLayerType(self):
        return LayerType(0)  # gopacket.LayerTypeZero

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        self.MaximumResponseDelay = int(t["v"][2]) * _MILLISECOND
        self.MulticastAddress = self._ip(t, 0, pkt)


class MLDv1MulticastListenerQueryMessage(MLDv1Message):
    """mldv1.go:87-132: Payload is data[20:] of a message longer than 20 bytes."""
    kind = 400 + 5
    ndp_kind = _lib.NDP_MLD1_QUERY
    _lt = LayerTypeMLDv1MulticastListenerQuery

    def IsGeneralQuery(self):
        return self.MulticastAddress == bytes(16)

    def IsSpecificQuery(self):
        return not self.IsGeneralQuery()


class MLDv1MulticastListenerReportMessage(MLDv1Message):
    """mldv1.go:134-150"""
    kind = 400 + 6
    ndp_kind = _lib.NDP_MLD1_REPORT
    _lt = LayerTypeMLDv1MulticastListenerReport


class MLDv1MulticastListenerDoneMessage(MLDv1Message):
    """mldv1.go:152-167"""
    kind = 400 + 7
    ndp_kind = _lib.NDP_MLD1_DONE
    _lt = LayerTypeMLDv1MulticastListenerDone


class MLDv2MulticastListenerQueryMessage(_NDPLayer):
    """mldv2.go:34-257. DecodeFromBytes sets no BaseLayer; NextLayerType is LayerTypeZero."""
    kind = 400 + 8
    ndp_kind = _lib.NDP_MLD2_QUERY
    _lt = LayerTypeMLDv2MulticastListenerQuery

    def __init__(self):
        self.MaximumResponseCode = 0
        self.MulticastAddress = b""
        self.SuppressRoutersideProcessing = False
        self.QueriersRobustnessVariable = self.QueriersQueryIntervalCode = self.NumberOfSources = 0
        self.SourceAddresses = []

    def NextLayerType(self):
        return LayerType(0)  # gopacket.LayerTypeZero

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        self.MaximumResponseCode = int(t["v"][2])
        self.MulticastAddress = self._ip(t, 0, pkt)
        self.SuppressRoutersideProcessing = bool(int(t["s_qrv"]) & 8)
        self.QueriersRobustnessVariable = int(t["s_qrv"]) & 7
        self.QueriersQueryIntervalCode = int(t["qqic"])
        self.NumberOfSources = int(t["count"])
        a = int(t["hdr_off"]) + 24
        self.SourceAddresses = [pkt[a + 16 * k:a + 16 * k + 16] for k in range(self.NumberOfSources)]

    def IsGeneralQuery(self):
        return self.MulticastAddress == bytes(16)

    def IsSpecificQuery(self):
        return not self.IsGeneralQuery()

    def QQI(self):
        """mldv2.go:194-203, its uint16 arithmetic included: 0x1000 << (exp + 3) keeps its low 16 bits."""
        data = self.QueriersQueryIntervalCode
        if data < 128:
            return _SECOND * data
        exp, mant = (data & 0x70) >> 4, data & 0x0F
        return _SECOND * ((mant | 0x1000 << (exp + 3)) & 0xFFFF)

    def MaximumResponseDelay(self):
        """mldv2.go:248-257 as written: a code below 0x8000 is returned as that
        many nanoseconds, and the shift is made in 16 bits."""
        code = self.MaximumResponseCode
        if code < 0x8000:
            return code
        exp, mant = (code & 0x7000) >> 12, code & 0x0FFF
        return _MILLISECOND * ((mant | 0x1000 << (exp + 3)) & 0xFFFF)


class MLDv2MulticastAddressRecordType(int):
    """mldv2.go:394-452"""

    def String(self):
        return _MLDV2_RECORD_NAMES.get(int(self), "UNKNOWN(%d)" % int(self))


(MLDv2MulticastAddressRecordTypeModeIsIncluded, MLDv2MulticastAddressRecordTypeModeIsExcluded,
 MLDv2MulticastAddressRecordTypeChangeToIncludeMode, MLDv2MulticastAddressRecordTypeChangeToExcludeMode,
 MLDv2MulticastAddressRecordTypeAllowNewSources, MLDv2MulticastAddressRecordTypeBlockOldSources) = (
    MLDv2MulticastAddressRecordType(k) for k in range(1, 7))
_MLDV2_RECORD_NAMES = {1: "MODE_IS_INCLUDE", 2: "MODE_IS_EXCLUDE", 3: "CHANGE_TO_INCLUDE_MODE",
                       4: "CHANGE_TO_EXCLUDE_MODE", 5: "ALLOW_NEW_SOURCES", 6: "BLOCK_OLD_SOURCES"}


class MLDv2MulticastAddressRecord:
    """mldv2.go:454-470"""

    def __init__(self, RecordType=0, AuxDataLen=0, N=0, MulticastAddress=b"", SourceAddresses=(), AuxiliaryData=b""):
        self.RecordType, self.AuxDataLen, self.N = MLDv2MulticastAddressRecordType(RecordType), AuxDataLen, N
        self.MulticastAddress, self.SourceAddresses = bytes(MulticastAddress), list(SourceAddresses)
        self.AuxiliaryData = bytes(AuxiliaryData)

    def _key(self):
        return (int(self.RecordType), self.AuxDataLen, self.N, self.MulticastAddress, self.SourceAddresses,
                self.AuxiliaryData)

    def __eq__(self, o):
        return isinstance(o, MLDv2MulticastAddressRecord) and self._key() == o._key()

    def __repr__(self):
        return "MLDv2MulticastAddressRecord%r" % (self._key(),)


class MLDv2MulticastListenerReportMessage(_NDPLayer):
    """mldv2.go:297-392. DecodeFromBytes sets no BaseLayer."""
    kind = 400 + 9
    ndp_kind = _lib.NDP_MLD2_REPORT
    _lt = LayerTypeMLDv2MulticastListenerReport

    def __init__(self):
        self.NumberOfMulticastAddressRecords = 0
        self.MulticastAddressRecords = []

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        self.NumberOfMulticastAddressRecords = int(t["count"])
        self.MulticastAddressRecords = []
        for e in entries:
            a, s, x, n = int(e["off"]), int(e["ext"]), int(e["aux_off"]), int(e["n"])
            self.MulticastAddressRecords.append(MLDv2MulticastAddressRecord(
                int(e["type"]), int(e["aux_data_len"]), n, pkt[a:a + 16], [pkt[s + 16 * k:s + 16 * k + 16] for k in range(n)],
                pkt[x:x + 4 * int(e["aux_data_len"])]))


NDP_LAYERS = (ICMPv6RouterSolicitation, ICMPv6RouterAdvertisement, ICMPv6NeighborSolicitation,
              ICMPv6NeighborAdvertisement, ICMPv6Redirect, MLDv1MulticastListenerQueryMessage,
              MLDv1MulticastListenerReportMessage, MLDv1MulticastListenerDoneMessage,
              MLDv2MulticastListenerQueryMessage, MLDv2MulticastListenerReportMessage)


# ---- layers/dhcpv4.go, dhcpv6.go, dhcpv6_options.go, ntp.go ----------------------
# A DecodingLayerParser that holds DHCPv4, DHCPv6 or NTP decodes the messages on
# the device after the TLS pass (gpk_svc_batch); the struct is filled from the
# packet's gpk_svc record, its gpk_svc_entry descriptors and the packet's bytes
# (_from_record). SerializeTo, the String() forms and the typed interpretation
# of option data (DHCPv6DUID, IA_NA contents) are not built.
LayerTypeNTP = _lt("NTP")
LayerTypeDHCPv4 = _lt("DHCPv4")
LayerTypeDHCPv6 = _lt("DHCPv6")


def _named_int(name, names, unknown="Unknown"):
    """An int subclass whose String() looks its value up in `names`."""
    return type(name, (int,), {"String": lambda self: names.get(int(self), unknown), "__slots__": ()})


def _export(cls, prefix, table):
    """prefix + suffix = cls(value) for every (value, suffix, text) of table; returns {value: text}."""
    for value, suffix, _ in table:
        globals()[prefix + suffix] = cls(value)
    return {value: text for value, _, text in table}


# dhcpv4.go:18-79: DHCPOp and DHCPMsgType
_DHCP_OP_NAMES, _DHCP_MSG_NAMES, _DHCP_OPT_NAMES, _DHCP6_MSG_NAMES, _DHCP6_OPT_NAMES = {}, {}, {}, {}, {}
DHCPOp = _named_int("DHCPOp", _DHCP_OP_NAMES)
DHCPMsgType = _named_int("DHCPMsgType", _DHCP_MSG_NAMES)
DHCPOpt = _named_int("DHCPOpt", _DHCP_OPT_NAMES)          # dhcpv4.go:262-474
DHCPv6MsgType = _named_int("DHCPv6MsgType", _DHCP6_MSG_NAMES)  # dhcpv6.go:18-72
DHCPv6Opt = _named_int("DHCPv6Opt", _DHCP6_OPT_NAMES)      # dhcpv6_options.go:17-594
DHCPMagic = 0x63825363
_DHCP_OP_NAMES.update(_export(DHCPOp, "DHCPOp", [(1, "Request", "Request"), (2, "Reply", "Reply")]))
_DHCP_MSG_NAMES.update(_export(DHCPMsgType, "DHCPMsgType", [
    (k, n, n) for k, n in enumerate("Unspecified Discover Offer Request Decline Ack Nak Release Inform".split())]))
_DHCP_OPT_NAMES.update(_export(DHCPOpt, "DHCPOpt", [
    (0, "Pad", "(padding)"), (1, "SubnetMask", "SubnetMask"), (2, "TimeOffset", "TimeOffset"), (3, "Router", "Router"),
    (4, "TimeServer", "rfc868"), (5, "NameServer", "ien116"), (6, "DNS", "DNS"), (7, "LogServer", "mitLCS"),
    (8, "CookieServer", "CookieServer"), (9, "LPRServer", "LPRServer"), (10, "ImpressServer", "ImpressServer"),
    (11, "ResLocServer", "ResourceLocationServer"), (12, "Hostname", "Hostname"), (13, "BootfileSize", "BootfileSize"),
    (14, "MeritDumpFile", "MeritDumpFile"), (15, "DomainName", "DomainName"), (16, "SwapServer", "SwapServer"),
    (17, "RootPath", "RootPath"), (18, "ExtensionsPath", "ExtensionsPath"), (19, "IPForwarding", "IPForwarding"),
    (20, "SourceRouting", "SourceRouting"), (21, "PolicyFilter", "PolicyFilter"), (22, "DatagramMTU", "DatagramMTU"),
    (23, "DefaultTTL", "DefaultTTL"), (24, "PathMTUAgingTimeout", "PathMTUAgingTimeout"),
    (25, "PathPlateuTableOption", "PathPlateuTableOption"), (26, "InterfaceMTU", "InterfaceMTU"),
    (27, "AllSubsLocal", "AllSubsLocal"), (28, "BroadcastAddr", "BroadcastAddress"), (29, "MaskDiscovery", "MaskDiscovery"),
    (30, "MaskSupplier", "MaskSupplier"), (31, "RouterDiscovery", "RouterDiscovery"), (32, "SolicitAddr", "SolicitAddr"),
    (33, "StaticRoute", "StaticRoute"), (34, "ARPTrailers", "ARPTrailers"), (35, "ARPTimeout", "ARPTimeout"),
    (36, "EthernetEncap", "EthernetEncap"), (37, "TCPTTL", "TCPTTL"), (38, "TCPKeepAliveInt", "TCPKeepAliveInt"),
    (39, "TCPKeepAliveGarbage", "TCPKeepAliveGarbage"), (40, "NISDomain", "NISDomain"), (41, "NISServers", "NISServers"),
    (42, "NTPServers", "NTPServers"), (43, "VendorOption", "VendorOption"), (44, "NetBIOSTCPNS", "NetBIOSOverTCPNS"),
    (45, "NetBIOSTCPDDS", "NetBiosOverTCPDDS"), (46, "NETBIOSTCPNodeType", "NetBIOSOverTCPNodeType"),
    (47, "NetBIOSTCPScope", "NetBIOSOverTCPScope"), (48, "XFontServer", "XFontServer"),
    (49, "XDisplayManager", "XDisplayManager"), (50, "RequestIP", "RequestIP"), (51, "LeaseTime", "LeaseTime"),
    (52, "ExtOptions", "ExtOpts"), (53, "MessageType", "MessageType"), (54, "ServerID", "ServerID"),
    (55, "ParamsRequest", "ParamsRequest"), (56, "Message", "Message"), (57, "MaxMessageSize", "MaxDHCPSize"),
    (58, "T1", "Timer1"), (59, "T2", "Timer2"), (60, "ClassID", "ClassID"), (61, "ClientID", "ClientID"),
    (119, "DomainSearch", "DomainSearch"), (120, "SIPServers", "SipServers"),
    (121, "ClasslessStaticRoute", "ClasslessStaticRoute"), (161, "MUDURLV4", "ManufacturerUsageDescriptionURL"),
    (255, "End", "(end)")]))
_DHCP6_MSG_NAMES.update(_export(DHCPv6MsgType, "DHCPv6MsgType", [
    (k, n, n) for k, n in enumerate(("Unspecified Solicit Advertise Request Confirm Renew Rebind Reply Release Decline "
                                     "Reconfigure InformationRequest RelayForward RelayReply").split())]))
_DHCP6_OPT_NAMES.update(_export(DHCPv6Opt, "DHCPv6Opt", [
    (1, "ClientID", "ClientID"), (2, "ServerID", "ServerID"), (3, "IANA", "IA_NA"), (4, "IATA", "IA_TA"),
    (5, "IAAddr", "IAAddr"), (6, "Oro", "Oro"), (7, "Preference", "Preference"), (8, "ElapsedTime", "ElapsedTime"),
    (9, "RelayMessage", "RelayMessage"), (11, "Auth", "Auth"), (12, "Unicast", "Unicast"), (13, "StatusCode", "StatusCode"),
    (14, "RapidCommit", "RapidCommit"), (15, "UserClass", "UserClass"), (16, "VendorClass", "VendorClass"),
    (17, "VendorOpts", "VendorOpts"), (18, "InterfaceID", "InterfaceID"), (19, "ReconfigureMessage", "ReconfigureMessage"),
    (20, "ReconfigureAccept", "ReconfigureAccept"), (21, "SIPServersDomainList", "SIPServersDomainList"),
    (22, "SIPServersAddressList", "SIPServersAddressList"), (23, "DNSServers", "DNSRecursiveNameServer"),
    (24, "DomainList", "DomainSearchList"), (25, "IAPD", "IdentityAssociationPrefixDelegation"),
    (26, "IAPrefix", "IAPDPrefix"), (27, "NISServers", "NISServers"), (28, "NISPServers", "NISv2Servers"),
    (29, "NISDomainName", "NISDomainName"), (30, "NISPDomainName", "NISv2DomainName"), (31, "SNTPServers", "SNTPServers"),
    (32, "InformationRefreshTime", "InformationRefreshTime"),
    (33, "BCMCSServerDomainNameList", "BCMCSControlServersDomainNameList"),
    (34, "BCMCSServerAddressList", "BCMCSControlServersAddressList"), (36, "GeoconfCivic", "CivicAddress"),
    (37, "RemoteID", "RelayAgentRemoteID"), (38, "SubscriberID", "RelayAgentSubscriberID"), (39, "ClientFQDN", "ClientFQDN"),
    (40, "PanaAgent", "PANAAuthenticationAgent"), (41, "NewPOSIXTimezone", "NewPOSIXTimezone"),
    (42, "NewTZDBTimezone", "NewTZDBTimezone"), (43, "EchoRequestOption", "EchoRequest"), (44, "LQQuery", "LeasequeryQuery"),
    (45, "CLTTime", "LeasequeryClientLastTransactionTime"), (46, "ClientData", "LeasequeryClientData"),
    (47, "LQRelayData", "LeasequeryRelayData"), (48, "LQClientLink", "LeasequeryClientLink"),
    (49, "MIP6HNIDF", "MIPv6HomeNetworkIDFQDN"), (50, "MIP6VDINF", "MIPv6VisitedHomeNetworkInformation"),
    (51, "V6LOST", "LoST Server"), (52, "CAPWAPACV6", "CAPWAPAccessControllerV6"), (53, "RelayID", "LeasequeryRelayID"),
    (54, "IPv6AddressMoS", "MoSIPv6Address"), (55, "IPv6FQDNMoS", "MoSDomainNameList"), (56, "NTPServer", "NTPServer"),
    (57, "V6AccessDomain", "AccessNetworkDomainName"), (58, "SIPUACSList", "SIPUserAgentConfigurationServiceDomains"),
    (59, "BootFileURL", "BootFileURL"), (60, "BootFileParam", "BootFileParameters"),
    (61, "ClientArchType", "ClientSystemArchitectureType"), (62, "NII", "ClientNetworkInterfaceIdentifier"),
    (63, "Geolocation", "Geolocation"), (64, "AFTRName", "AFTRName"), (65, "ERPLocalDomainName", "AFTRName"),
    (66, "RSOO", "RSOOption"), (67, "PDExclude", "PrefixExclude"), (68, "VSS", "VirtualSubnetSelection"),
    (69, "MIP6IDINF", "MIPv6IdentifiedHomeNetworkInformation"), (70, "MIP6UDINF", "MIPv6UnrestrictedHomeNetworkInformation"),
    (71, "MIP6HNP", "MIPv6HomeNetworkPrefix"), (72, "MIP6HAA", "MIPv6HomeAgentAddress"), (73, "MIP6HAF", "MIPv6HomeAgentFQDN"),
    (74, "RDNSSSelection", "RDNSSSelection"), (75, "KRBPrincipalName", "KerberosPrincipalName"),
    (76, "KRBRealmName", "KerberosRealmName"), (77, "KRBKDC", "KerberosKDC"),
    (79, "ClientLinkLayerAddress", "ClientLinkLayerAddress"), (80, "LinkAddress", "LinkAddress"), (81, "RADIUS", "RADIUS"),
    (82, "SolMaxRt", "SolMaxRt"), (83, "InfMaxRt", "InfMaxRt"), (84, "AddrSel", "AddressSelection"),
    (85, "AddrSelTable", "AddressSelectionTable"), (86, "V6PCPServer", "PCPServer"), (87, "DHCPv4Message", "DHCPv4Message"),
    (88, "DHCPv4OverDHCPv6Server", "DHCP4o6ServerAddress"), (89, "S46Rule", "S46Rule"), (90, "S46BR", "S46BR"),
    (91, "S46DMR", "S46DMR"), (92, "S46V4V4Bind", "S46IPv4IPv6AddressBinding"), (93, "S46PortParameters", "S46PortParameters"),
    (94, "S46ContMAPE", "S46MAPEContainer"), (95, "S46ContMAPT", "S46MAPTContainer"),
    (96, "S46ContLW", "S46Lightweight4Over6Container"), (97, "4RD", "4RD"), (98, "4RDMapRule", "4RDMapRule"),
    (99, "4RDNonMapRule", "4RDNonMapRule"), (100, "LQBaseTime", "LQBaseTime"), (101, "LQStartTime", "LQStartTime"),
    (102, "LQEndTime", "LQEndTime"), (103, "CaptivePortal", "CaptivePortal"), (104, "MPLParameters", "MPLParameterConfiguration"),
    (105, "ANIATT", "ANIAccessTechnologyType"), (106, "ANINetworkName", "ANINetworkName"), (107, "ANIAPName", "ANIAccessPointName"),
    (108, "ANIAPBSSID", "ANIAccessPointBSSID"), (109, "ANIOperatorID", "ANIOperatorIdentifier"),
    (110, "ANIOperatorRealm", "ANIOperatorRealm"), (111, "S46Priority", "S64Priority"),
    (112, "MUDURLV6", "ManufacturerUsageDescriptionURL"), (113, "V6Prefix64", "V6Prefix64"),
    (135, "RelayPort", "RelayPort"), (136, "V6ZeroTouchRedirect", "ZeroTouch"), (143, "IPV6AddressANDSF", "ANDSFIPv6Address")]))
_DHCP6_OPT_NAMES.update(_export(DHCPv6Opt, "DHCPv6OptF", [  # the failover options of RFC 8156
    (114 + k, s, "Failover" + n) for k, (s, n) in enumerate([
        ("BindingStatus", "BindingStatus"), ("ConnectFlags", "ConnectFlags"), ("DNSRemovalInfo", "DNSRemovalInfo"),
        ("DNSHostName", "DNSHostName"), ("DNSZoneName", "DNSZoneName"), ("DNSFlags", "DNSFlags"),
        ("ExpirationTime", "ExpirationTime"), ("MaxUnacknowledgedBNDUPD", "MaxUnacknowledgedBNDUPDMessages"),
        ("MCLT", "MaximumClientLeadTime"), ("PartnerLifetime", "PartnerLifetime"),
        ("PartnerLifetimeSent", "PartnerLifetimeSent"), ("PartnerDownTime", "PartnerDownTime"),
        ("PartnerRawCltTime", "PartnerRawClientLeadTime"), ("ProtocolVersion", "ProtocolVersion"),
        ("KeepaliveTime", "KeepaliveTime"), ("ReconfigureData", "ReconfigureData"), ("RelationshipName", "RelationshipName"),
        ("ServerFlags", "ServerFlags"), ("ServerState", "ServerState"), ("StartTimeOfState", "StartTimeOfState"),
        ("StateExpirationTime", "StateExpirationTime")])]))


class DHCPOption:
    """dhcpv4.go:478-482. A Pad has Length 0 and no Data."""

    def __init__(self, Type=0, Length=0, Data=b""):
        self.Type, self.Length, self.Data = DHCPOpt(Type), int(Length), bytes(Data)

    def __eq__(self, o):
        return isinstance(o, DHCPOption) and (int(self.Type), self.Length, self.Data) == (int(o.Type), o.Length, o.Data)

    def __repr__(self):
        return "DHCPOption(%s, %d, %r)" % (self.Type.String(), self.Length, self.Data)


class DHCPOptions(list):
    """dhcpv4.go:476"""


class DHCPv6Option:
    """dhcpv6_options.go:559-563"""

    def __init__(self, Code=0, Length=0, Data=b""):
        self.Code, self.Length, self.Data = DHCPv6Opt(Code), int(Length), bytes(Data)

    def __eq__(self, o):
        return isinstance(o, DHCPv6Option) and (int(self.Code), self.Length, self.Data) == (int(o.Code), o.Length, o.Data)

    def __repr__(self):
        return "DHCPv6Option(%s, %d, %r)" % (self.Code.String(), self.Length, self.Data)


class DHCPv6Options(list):
    """dhcpv6_options.go:557"""


class _SvcLayer(BaseLayer):
    _lt = None
    _next = LayerTypePayload

    def DecodeFromBytes(self, data, df):
        raise NotImplementedError("DHCPv4, DHCPv6 and NTP decode through a DecodingLayerParser (DecodeLayers / DecodeBatch)")

    def LayerType(self):
        return self._lt

    def CanDecode(self):
        return LayerClass([self._lt])

    def NextLayerType(self):
        return self._next

    def _base(self, t, pkt):
        h = int(t["hdr_off"])
        self.Contents = pkt[h:h + int(t["contents_len"])]
        self.Payload = b""


class DHCPv4(_SvcLayer):
    """dhcpv4.go:84-101, 126-184"""
    kind = 500 + 0
    svc_kind = _lib.SVC_DHCP4
    _lt = LayerTypeDHCPv4

    def __init__(self):
        self.Operation, self.HardwareType, self.HardwareLen, self.RelayHops = DHCPOp(0), 0, 0, 0
        self.Xid = self.Secs = self.Flags = 0
        self.ClientIP = self.YourClientIP = self.NextServerIP = self.RelayAgentIP = b""
        self.ClientHWAddr = self.ServerName = self.File = b""
        self.Options = DHCPOptions()

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        h, b, v = int(t["hdr_off"]), t["b"], t["v"]
        self.Operation, self.HardwareType, self.HardwareLen, self.RelayHops = DHCPOp(int(b[0])), int(b[1]), int(b[2]), int(b[3])
        self.Xid, self.Secs, self.Flags = int(v[0]), int(v[1]) & 0xffff, int(v[1]) >> 16
        ips = v[2:6].astype("<u4").tobytes()
        self.ClientIP, self.YourClientIP, self.NextServerIP, self.RelayAgentIP = (ips[4 * k:4 * k + 4] for k in range(4))
        self.ClientHWAddr = pkt[h + 28:h + 28 + self.HardwareLen]
        self.ServerName, self.File = pkt[h + 44:h + 108], pkt[h + 108:h + 236]
        self.Options = DHCPOptions(
            DHCPOption(int(e["code"]), int(e["length"]), pkt[int(e["off"]):int(e["off"]) + int(e["length"])]) for e in entries)


class DHCPv6(_SvcLayer):
    """dhcpv6.go:74-124"""
    kind = 500 + 1
    svc_kind = _lib.SVC_DHCP6
    _lt = LayerTypeDHCPv6

    def __init__(self):
        self.MsgType, self.HopCount = DHCPv6MsgType(0), 0
        self.LinkAddr = self.PeerAddr = self.TransactionID = b""
        self.Options = DHCPv6Options()

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        b, v = t["b"], t["v"]
        self.MsgType, self.HopCount = DHCPv6MsgType(int(b[0])), int(b[1])
        self.LinkAddr = self.PeerAddr = self.TransactionID = b""
        if int(self.MsgType) in (12, 13):
            self.LinkAddr, self.PeerAddr = pkt[int(v[1]):int(v[1]) + 16], pkt[int(v[2]):int(v[2]) + 16]
        else:
            self.TransactionID = int(v[0]).to_bytes(3, "big")
        self.Options = DHCPv6Options(
            DHCPv6Option(int(e["code"]), int(e["length"]), pkt[int(e["off"]):int(e["off"]) + int(e["length"])])
            for e in entries)


class NTP(_SvcLayer):
    """ntp.go:166-253, 294-347. The scalar types (NTPLeapIndicator, NTPVersion,
    NTPMode, NTPStratum, NTPLog2Seconds, NTPFixed16Seconds, NTPReferenceID,
    NTPTimestamp) are plain ints; Poll and Precision are signed."""
    kind = 500 + 2
    svc_kind = _lib.SVC_NTP
    _lt = LayerTypeNTP
    _next = LayerType(0)

    def __init__(self):
        self.LeapIndicator = self.Version = self.Mode = self.Stratum = self.Poll = self.Precision = 0
        self.RootDelay = self.RootDispersion = self.ReferenceID = 0
        self.ReferenceTimestamp = self.OriginTimestamp = self.ReceiveTimestamp = self.TransmitTimestamp = 0
        self.ExtensionBytes = b""

    def _from_record(self, t, entries, pkt):
        self._base(t, pkt)
        h, b, v = int(t["hdr_off"]), t["b"], t["v"]
        self.LeapIndicator, self.Version, self.Mode, self.Stratum = (int(x) for x in b)
        s8 = lambda x: x - 256 if x > 127 else x  # noqa: E731
        self.Poll, self.Precision = s8(int(v[0]) & 0xff), s8(int(v[0]) >> 8 & 0xff)
        self.RootDelay, self.RootDispersion, self.ReferenceID = int(v[1]), int(v[2]), int(v[3])
        (self.ReferenceTimestamp, self.OriginTimestamp, self.ReceiveTimestamp,
         self.TransmitTimestamp) = struct.unpack(">4Q", pkt[h + 16:h + 48])  # the record does not carry them
        self.ExtensionBytes = pkt[int(v[4]):int(v[4]) + int(v[5])]


SVC_LAYERS = (DHCPv4, DHCPv6, NTP)


# ---- layers/dns.go ------------------------------------------------------------------
# A DecodingLayerParser that holds layers.DNS decodes the messages on the device
# after the six-layer decode and the control pass (gpk_dns_batch); the struct is
# filled from the packet's gpk_dns record, its gpk_dns_rr entries, the name arena
# and the packet's bytes (_from_record).
class DNSClass(int):
    pass


class DNSType(int):
    pass


class DNSOpCode(int):
    pass


class DNSResponseCode(int):
    pass


DNSClassIN, DNSClassCS, DNSClassCH, DNSClassHS, DNSClassAny = (DNSClass(x) for x in (1, 2, 3, 4, 255))
(DNSTypeA, DNSTypeNS, DNSTypeMD, DNSTypeMF, DNSTypeCNAME, DNSTypeSOA, DNSTypeMB, DNSTypeMG, DNSTypeMR, DNSTypeNULL,
 DNSTypeWKS, DNSTypePTR, DNSTypeHINFO, DNSTypeMINFO, DNSTypeMX, DNSTypeTXT) = (DNSType(x) for x in range(1, 17))
(DNSTypeAAAA, DNSTypeSRV, DNSTypeNAPTR, DNSTypeOPT, DNSTypeRRSIG, DNSTypeDNSKEY, DNSTypeSVCB, DNSTypeHTTPS,
 DNSTypeURI) = (DNSType(x) for x in (28, 33, 35, 41, 46, 48, 64, 65, 256))
(DNSOpCodeQuery, DNSOpCodeIQuery, DNSOpCodeStatus, DNSOpCodeNotify, DNSOpCodeUpdate) = (
    DNSOpCode(x) for x in (0, 1, 2, 4, 5))
(DNSResponseCodeNoErr, DNSResponseCodeFormErr, DNSResponseCodeServFail, DNSResponseCodeNXDomain,
 DNSResponseCodeNotImp, DNSResponseCodeRefused, DNSResponseCodeYXDomain, DNSResponseCodeYXRRSet,
 DNSResponseCodeNXRRSet, DNSResponseCodeNotAuth, DNSResponseCodeNotZone) = (DNSResponseCode(x) for x in range(11))
(DNSResponseCodeBadVers, DNSResponseCodeBadSig, DNSResponseCodeBadKey, DNSResponseCodeBadTime,
 DNSResponseCodeBadMode, DNSResponseCodeBadName, DNSResponseCodeBadAlg, DNSResponseCodeBadTruc,
 DNSResponseCodeBadCookie) = (DNSResponseCode(x) for x in (16, 16, 17, 18, 19, 20, 21, 22, 23))


@dataclass
class DNSQuestion:
    Name: bytes = b""
    Type: DNSType = DNSType(0)
    Class: DNSClass = DNSClass(0)


@dataclass
class DNSSOA:
    MName: bytes = b""
    RName: bytes = b""
    Serial: int = 0
    Refresh: int = 0
    Retry: int = 0
    Expire: int = 0
    Minimum: int = 0


@dataclass
class DNSSRV:
    Priority: int = 0
    Weight: int = 0
    Port: int = 0
    Name: bytes = b""


@dataclass
class DNSMX:
    Preference: int = 0
    Name: bytes = b""


@dataclass
class DNSURI:
    Priority: int = 0
    Weight: int = 0
    Target: bytes = b""


@dataclass
class DNSNAPTR:
    Order: int = 0
    Preference: int = 0
    Flags: bytes = b""
    Service: bytes = b""
    Regexp: bytes = b""
    Replacement: bytes = b""


@dataclass
class DNSOPT:
    Code: int = 0
    Data: bytes = b""


@dataclass
class DNSSvcParam:
    Key: int = 0
    Value: bytes = b""


@dataclass
class DNSSVCB:
    Priority: int = 0
    Target: bytes = b""
    Params: list = field(default_factory=list)


@dataclass
class DNSRRSIG:
    TypeCovered: DNSType = DNSType(0)
    Algorithm: int = 0
    Labels: int = 0
    OriginalTTL: int = 0
    Expiration: int = 0
    Inception: int = 0
    KeyTag: int = 0
    SignerName: bytes = b""
    Signature: bytes = b""


@dataclass
class DNSKEY:
    Flags: int = 0
    Protocol: int = 0
    Algorithm: int = 0
    PublicKey: bytes = b""


@dataclass
class DNSResourceRecord:
    Name: bytes = b""
    Type: DNSType = DNSType(0)
    Class: DNSClass = DNSClass(0)
    TTL: int = 0
    DataLength: int = 0
    Data: bytes = b""
    IP: bytes = b""
    NS: bytes = b""
    CNAME: bytes = b""
    PTR: bytes = b""
    TXTs: list = field(default_factory=list)
    SOA: DNSSOA = field(default_factory=DNSSOA)
    SRV: DNSSRV = field(default_factory=DNSSRV)
    MX: DNSMX = field(default_factory=DNSMX)
    NAPTR: DNSNAPTR = field(default_factory=DNSNAPTR)
    OPT: list = field(default_factory=list)
    RRSIG: DNSRRSIG = field(default_factory=DNSRRSIG)
    DNSKEY: DNSKEY = field(default_factory=DNSKEY)
    SVCB: DNSSVCB = field(default_factory=DNSSVCB)
    URI: DNSURI = field(default_factory=DNSURI)
    TXT: bytes = b""


def _dns_entry(r, names, pkt):
    """A DNSQuestion or DNSResourceRecord from a gpk_dns_rr entry, the name
    arena and the packet. The lists (TXTs, OPT, SvcParams) are sliced out of
    the packet with the walk the device has validated (r["count"] items)."""
    def arena(off, ln):
        o = int(r[off])
        return bytes(names[o:o + int(r[ln])])
    name = arena("name_off", "name_len")
    typ = int(r["type"])
    if int(r["section"]) == _lib.DNS_SEC_QUESTION:
        return DNSQuestion(name, DNSType(typ), DNSClass(int(r["cls"])))
    d, dl = int(r["data_off"]), int(r["data_length"])
    data = bytes(pkt[d:d + dl])
    rr = DNSResourceRecord(name, DNSType(typ), DNSClass(int(r["cls"])), int(r["ttl"]), dl, data)
    if not dl:  # dns.go:1080: decodeRData is skipped
        return rr
    v = [int(x) for x in r["v"]]
    rname = arena("rname_off", "rname_len")

    def items(at, width):  # `count` items of a `width`-byte length field behind a (width - 1) * 2-byte code
        out, head = [], 2 * (width - 1)
        for _ in range(int(r["count"])):
            ln = int.from_bytes(pkt[at + head:at + head + width], "big")
            out.append((int.from_bytes(pkt[at:at + head], "big"), bytes(pkt[at + head + width:at + head + width + ln])))
            at += head + width + ln
        return out
    if typ in (1, 28):
        rr.IP = data
    elif typ in (16, 13):
        rr.TXT = data
        rr.TXTs = [x for _, x in items(d, 1)]
    elif typ == 2:
        rr.NS = rname
    elif typ == 5:
        rr.CNAME = rname
    elif typ == 12:
        rr.PTR = rname
    elif typ == 6:
        rr.SOA = DNSSOA(rname, arena("rname2_off", "rname2_len"), *v[:5])
    elif typ == 15:
        rr.MX = DNSMX(v[0], rname)
    elif typ == 256:
        rr.URI = DNSURI(v[0], v[1], data[4:])
    elif typ == 33:
        rr.SRV = DNSSRV(v[0], v[1], v[2], rname)
    elif typ == 35:
        rr.NAPTR = DNSNAPTR(v[0], v[1], bytes(pkt[v[2]:v[2] + v[3]]), bytes(pkt[v[4]:v[4] + v[5]]),
                            bytes(pkt[v[6]:v[6] + v[7]]), rname)
    elif typ == 41:
        rr.OPT = [DNSOPT(c, x) for c, x in items(d, 2)]
    elif typ == 46:
        rr.RRSIG = DNSRRSIG(DNSType(v[0]), v[1], v[2], v[3], v[4], v[5], v[6], rname, bytes(pkt[v[7]:v[7] + v[8]]))
    elif typ == 48:
        rr.DNSKEY = DNSKEY(v[0], v[1], v[2], data[4:])
    elif typ in (64, 65):
        rr.SVCB = DNSSVCB(v[0], rname, [DNSSvcParam(k, x) for k, x in items(v[1], 2)])
    return rr


class DNS(BaseLayer):
    """dns.go:284-436. Payload() is nil: nothing follows a DNS layer."""
    kind = 300
    dns_kind = _lib.DNS_KIND

    def __init__(self):
        self._reset()

    def _reset(self):
        self.ID = 0
        self.QR = self.AA = self.TC = self.RD = self.RA = False
        self.OpCode = DNSOpCode(0)
        self.Z = 0
        self.ResponseCode = DNSResponseCode(0)
        self.QDCount = self.ANCount = self.NSCount = self.ARCount = 0
        self.Questions, self.Answers, self.Authorities, self.Additionals = [], [], [], []
        self.Contents = self.Payload = b""

    def LayerType(self):
        return LayerTypeDNS

    def CanDecode(self):
        return LayerClass([LayerTypeDNS])

    def NextLayerType(self):
        return LayerTypePayload

    def LayerPayload(self):
        return b""

    def DecodeFromBytes(self, data, df):
        raise NotImplementedError("DNS decodes through a DecodingLayerParser (DecodeLayers / DecodeBatch)")

    def _from_record(self, t, rrs, names, pkt):
        """t: the gpk_dns record (decoded, not dropped); rrs: its entries; names: the arena."""
        self._reset()
        f2, f3 = int(t["flags2"]), int(t["flags3"])
        self.ID = int(t["id"])
        self.QR, self.OpCode = bool(f2 & 0x80), DNSOpCode(f2 >> 3 & 0xF)
        self.AA, self.TC, self.RD, self.RA = bool(f2 & 4), bool(f2 & 2), bool(f2 & 1), bool(f3 & 0x80)
        self.Z = f3 >> 4 & 7
        self.ResponseCode = DNSResponseCode(int(t["response_code"]))
        self.QDCount, self.ANCount = int(t["qdcount"]), int(t["ancount"])
        self.NSCount, self.ARCount = int(t["nscount"]), int(t["arcount"])
        h = int(t["hdr_off"])
        self.Contents = bytes(pkt[h:h + int(t["len"])])
        sections = (self.Questions, self.Answers, self.Authorities, self.Additionals)
        for r in rrs:
            sections[int(r["section"])].append(_dns_entry(r, names, pkt))


# ---- layers/tls.go, tls_handshake.go, tls_alert.go, tls_cipherspec.go, tls_appdata.go ------------
# A DecodingLayerParser that holds layers.TLS decodes the messages on the device
# after the DNS pass (gpk_tls_batch); the struct is filled from the packet's
# gpk_tls record, its gpk_tls_rec and gpk_tls_hello entries and the packet's
# bytes (_from_record). TLS.SerializeTo is not built.
class TLSType(int):
    """tls.go:17-42"""

    def String(self):
        return {20: "Change Cipher Spec", 21: "Alert", 22: "Handshake", 23: "Application Data"}.get(int(self), "Unknown")

    __str__ = String


class TLSVersion(int):
    """tls.go:45-65"""

    def String(self):
        return {0x0200: "SSL 2.0", 0x0300: "SSL 3.0", 0x0301: "TLS 1.0", 0x0302: "TLS 1.1", 0x0303: "TLS 1.2",
                0x0304: "TLS 1.3"}.get(int(self), "Unknown")

    __str__ = String


class TLSAlertLevel(int):
    """tls_alert.go:17,98-107"""

    def String(self):
        return {1: "Warning", 2: "Fatal"}.get(int(self), "Unknown(%d)" % int(self))

    __str__ = String


_TLS_ALERT_DESCR = {
    0: "close_notify", 10: "unexpected_message", 20: "bad_record_mac", 21: "decryption_failed_RESERVED",
    22: "record_overflow", 30: "decompression_failure", 40: "handshake_failure", 41: "no_certificate_RESERVED",
    42: "bad_certificate", 43: "unsupported_certificate", 44: "certificate_revoked", 45: "certificate_expired",
    46: "certificate_unknown", 47: "illegal_parameter", 48: "unknown_ca", 49: "access_denied", 50: "decode_error",
    51: "decrypt_error", 60: "export_restriction_RESERVED", 70: "protocol_version", 71: "insufficient_security",
    80: "internal_error", 90: "user_canceled", 100: "no_renegotiation", 110: "unsupported_extension"}


class TLSAlertDescr(int):
    """tls_alert.go:20,110-165"""

    def String(self):
        return _TLS_ALERT_DESCR.get(int(self), "Unknown")

    __str__ = String


class TLSchangeCipherSpec(int):
    """tls_cipherspec.go:16,57-64"""

    def String(self):
        return "Change Cipher Spec Message" if int(self) == 1 else "Unknown"

    __str__ = String


TLSChangeCipherSpec, TLSAlert, TLSHandshake, TLSApplicationData, TLSUnknown = (TLSType(x) for x in (20, 21, 22, 23, 255))
TLSAlertWarning, TLSAlertFatal, TLSAlertUnknownLevel = (TLSAlertLevel(x) for x in (1, 2, 255))
TLSAlertUnknownDescription = TLSAlertDescr(255)
TLSChangecipherspecMessage, TLSChangecipherspecUnknown = TLSchangeCipherSpec(1), TLSchangeCipherSpec(255)
(TLSHandshakeHelloRequest, TLSHandshakeClientHello, TLSHandshakeServerHello, TLSHandsharkHelloVerirfyRequest,
 TLSHandshakeCertificate, TLSHandshakeServerKeyExchange, TLSHandshakeCertificateRequest, TLSHandshakeServerHelloDone,
 TLSHandshakeCertificateVerify, TLSHandshakeClientKeyExchange, TLSHandshakeFinished) = (0, 1, 2, 3, 11, 12, 13, 14, 15,
                                                                                        16, 20)


@dataclass
class TLSRecordHeader:
    ContentType: TLSType = TLSType(0)
    Version: TLSVersion = TLSVersion(0)
    Length: int = 0


@dataclass
class TLSChangeCipherSpecRecord:
    TLSRecordHeader: TLSRecordHeader = field(default_factory=TLSRecordHeader)
    Message: TLSchangeCipherSpec = TLSchangeCipherSpec(0)


@dataclass
class TLSAppDataRecord:
    TLSRecordHeader: TLSRecordHeader = field(default_factory=TLSRecordHeader)
    Payload: Optional[bytes] = None


@dataclass
class TLSAlertRecord:
    TLSRecordHeader: TLSRecordHeader = field(default_factory=TLSRecordHeader)
    Level: TLSAlertLevel = TLSAlertLevel(0)
    Description: TLSAlertDescr = TLSAlertDescr(0)
    EncryptedMsg: Optional[bytes] = None


@dataclass
class TLSHandshakeRecordClientHello:
    HandshakeType: int = 0
    Length: int = 0
    ProtocolVersion: TLSVersion = TLSVersion(0)
    Random: Optional[bytes] = None
    SessionIDLength: int = 0
    SessionID: Optional[bytes] = None
    CipherSuitsLength: int = 0
    CipherSuits: Optional[bytes] = None
    CompressionMethodsLength: int = 0
    CompressionMethods: Optional[bytes] = None
    ExtensionsLength: int = 0
    Extensions: Optional[bytes] = None
    SNI: Optional[bytes] = None


@dataclass
class TLSHandshakeRecordClientKeyChange:
    pass


@dataclass
class TLSHandshakeRecord:
    TLSRecordHeader: TLSRecordHeader = field(default_factory=TLSRecordHeader)
    ClientHello: TLSHandshakeRecordClientHello = field(default_factory=TLSHandshakeRecordClientHello)
    ClientKeyChange: TLSHandshakeRecordClientKeyChange = field(default_factory=TLSHandshakeRecordClientKeyChange)


def _tls_hello(h, pkt):
    """A TLSHandshakeRecordClientHello from a gpk_tls_hello entry and the packet's bytes."""
    def cut(off, n):
        o = int(h[off])
        return bytes(pkt[o:o + n])
    sid, cs = int(h["session_id_length"]), int(h["cipher_suits_length"])
    cm, ext = int(h["compression_methods_length"]), int(h["extensions_length"])
    return TLSHandshakeRecordClientHello(
        int(h["handshake_type"]), int(h["length"]), TLSVersion(int(h["protocol_version"])), cut("random_off", 32), sid,
        cut("session_id_off", sid), cs, cut("cipher_suits_off", cs), cm, cut("compression_methods_off", cm), ext,
        cut("extensions_off", ext), cut("sni_off", int(h["sni_len"])) if int(h["has_sni"]) else None)


class TLS(BaseLayer):
    """tls.go:84-209. Payload() is nil: nothing follows a TLS layer."""
    kind = 301
    tls_kind = _lib.TLS_KIND

    def __init__(self):
        self._reset()

    def _reset(self):
        self.ChangeCipherSpec, self.Handshake, self.AppData, self.Alert = [], [], [], []
        self.Contents = self.Payload = b""

    def LayerType(self):
        return LayerTypeTLS

    def CanDecode(self):
        return LayerClass([LayerTypeTLS])

    def NextLayerType(self):
        return LayerType(0)  # gopacket.LayerTypeZero

    def LayerPayload(self):
        return b""

    def DecodeFromBytes(self, data, df):
        raise NotImplementedError("TLS decodes through a DecodingLayerParser (DecodeLayers / DecodeBatch)")

    def SerializeTo(self, b, opts):
        raise NotImplementedError("TLS.SerializeTo is not built")

    def _from_record(self, t, recs, hellos, pkt):
        """t: the gpk_tls record (decoded, not dropped); recs, hellos: its entries."""
        self._reset()
        end = int(t["hdr_off"]) + int(t["len"])
        for r in recs:
            ct, o, n = int(r["content_type"]), int(r["body_off"]), int(r["length"])
            hdr = TLSRecordHeader(TLSType(ct), TLSVersion(int(r["version"])), n)
            if ct == 20:
                self.ChangeCipherSpec.append(TLSChangeCipherSpecRecord(hdr, TLSchangeCipherSpec(int(r["v0"]))))
            elif ct == 21:
                self.Alert.append(TLSAlertRecord(hdr, TLSAlertLevel(int(r["v0"])), TLSAlertDescr(int(r["v1"])),
                                                 None if n == 2 else bytes(pkt[o:o + n])))
            elif ct == 22:
                rec = TLSHandshakeRecord(hdr)
                if int(r["hs"]) == _lib.TLS_HS_CLIENT_HELLO:
                    rec.ClientHello = _tls_hello(hellos[int(r["hello"])], pkt)
                self.Handshake.append(rec)
            else:
                self.AppData.append(TLSAppDataRecord(hdr, bytes(pkt[o:o + n])))
            self.Contents = bytes(pkt[o - 5:end])  # tls.go:139: reset for every record, the last one's stays
