// gpk_control_rules.h — the per-packet rules of gpk_control_batch, shared by the
// kernels and gpk_control_batch_host (one __host__ __device__ source, so the CPU
// suite checks the code the device runs).
//
//   candidate      tun::candidate of gpk_tunnel_rules.h over the parser's tables:
//                  the payload and next type of the last decoded layer
//   decode_icmp4 / decode_icmp6 / decode_echo / decode_arp
//                  DecodeFromBytes of layers/{icmp4,icmp6,icmp6msg,arp}.go. Every
//                  slice expression is guarded by the length check in front of
//                  it, so no run-time panic exists in the four.
//   control        one packet: candidate, first layer, the rest of the loop
//                  (layers_decoder.go:60-79), whether an ICMPv6 sum has a
//                  network layer for its pseudo-header
//   network_layer / start_value
//                  where that layer's addresses are, and computeChecksum's
//                  start value from their words (the sum step reads them)
#pragma once
#include <stdint.h>

#include "../../include/gpk_control.h"
#include "gpk_tunnel_rules.h"

namespace gpk {
namespace ctl {

using tun::be16;

GPK_HD uint32_t kind_of_type(int32_t lt) {
  return lt == GPK_LT_ICMPV4        ? GPK_CTL_ICMP4
         : lt == GPK_LT_ICMPV6      ? GPK_CTL_ICMP6
         : lt == GPK_LT_ICMPV6_ECHO ? GPK_CTL_ICMP6ECHO
         : lt == GPK_LT_ARP         ? GPK_CTL_ARP
                                    : 0u;
}

// A gpk_control being decoded, one dword per field (as tun::Tun): it stays in
// registers and is packed once, at the store.
struct Ctl {
  uint32_t kind, err, status, nlayers, a0, a1, hdr_off, contents_len, payload_off, payload_len;
  int32_t unsupported;
  uint32_t lt0, lt1, lt2, typecode, checksum, correct, id, seq, addr_type, protocol, hw, prot, op;
  int32_t next;
  uint32_t sum_init;
};

GPK_HD Ctl ctl_init(uint32_t kind, uint32_t hdr_off) {
  Ctl c;
  c.kind = kind;
  c.hdr_off = hdr_off;
  c.err = c.status = c.nlayers = c.a0 = c.a1 = c.contents_len = c.payload_off = c.payload_len = 0;
  c.unsupported = 0;
  c.lt0 = c.lt1 = c.lt2 = c.typecode = c.checksum = c.correct = c.id = c.seq = 0;
  c.addr_type = c.protocol = c.hw = c.prot = c.op = 0;
  c.next = 0;
  c.sum_init = 0;
  return c;
}

// the packed record (include/gpk_control.h), as 16 little-endian dwords
GPK_HD void ctl_store(gpk_control* dst, const Ctl& c) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = c.kind | c.err << 8 | c.status << 16 | c.nlayers << 24;
  w[1] = c.a0;
  w[2] = c.a1;
  w[3] = c.hdr_off;
  w[4] = c.contents_len;
  w[5] = c.payload_off;
  w[6] = c.payload_len;
  w[7] = (uint32_t)c.unsupported;
  w[8] = c.lt0 | c.lt1 << 16;
  w[9] = c.lt2 | c.typecode << 16;
  w[10] = c.checksum | c.correct << 16;
  w[11] = c.id | c.seq << 16;
  w[12] = c.addr_type | c.protocol << 16;
  w[13] = c.hw | c.prot << 8 | c.op << 16;
  w[14] = (uint32_t)c.next;
  w[15] = c.sum_init;
}

GPK_HD void fail(Ctl& c, uint32_t code, uint32_t a0 = 0, uint32_t a1 = 0) {  // every error site sets Truncated
  c = ctl_init(c.kind, c.hdr_off);
  c.err = code;
  c.a0 = a0;
  c.a1 = a1;
  c.status = GPK_CTL_ST_TRUNCATED;
}

GPK_HD void done(Ctl& c, uint32_t contents, uint32_t len, int32_t next) {
  c.contents_len = contents;
  c.payload_off = c.hdr_off + contents;
  c.payload_len = len - contents;
  c.next = next;
}

// icmp4.go:221-232; NextLayerType is Payload (:261-263)
GPK_HD void decode_icmp4(const uint8_t* d, uint32_t len, Ctl& c) {
  if (len < 8) return fail(c, GPK_CTL_ERR_ICMP4_SHORT);
  c.typecode = be16(d);
  c.checksum = be16(d + 2);
  c.id = be16(d + 4);
  c.seq = be16(d + 6);
  done(c, 8, len, GPK_LT_PAYLOAD);
}

// ICMPv6.NextLayerType, icmp6.go:230-261
GPK_HD int32_t icmp6_next(uint32_t type, uint32_t payload_len) {
  switch (type) {
    case 128:
    case 129: return GPK_LT_ICMPV6_ECHO;
    case 133: return GPK_LT_ICMPV6_ROUTER_SOLICITATION;
    case 134: return GPK_LT_ICMPV6_ROUTER_ADVERTISEMENT;
    case 135: return GPK_LT_ICMPV6_NEIGHBOR_SOLICITATION;
    case 136: return GPK_LT_ICMPV6_NEIGHBOR_ADVERTISEMENT;
    case 137: return GPK_LT_ICMPV6_REDIRECT;
    case 130: return payload_len > 20 ? GPK_LT_MLDV2_QUERY : GPK_LT_MLDV1_QUERY;  // only the size differs
    case 132: return GPK_LT_MLDV1_DONE;
    case 131: return GPK_LT_MLDV1_REPORT;
    case 143: return GPK_LT_MLDV2_REPORT;
    default: return GPK_LT_PAYLOAD;
  }
}

// icmp6.go:189-198
GPK_HD void decode_icmp6(const uint8_t* d, uint32_t len, Ctl& c) {
  if (len < 4) return fail(c, GPK_CTL_ERR_ICMP6_SHORT);
  c.typecode = be16(d);
  c.checksum = be16(d + 2);
  done(c, 4, len, icmp6_next(d[0], len - 4));
}

// icmp6msg.go:155-164: no BaseLayer is set, so Contents and Payload stay empty
GPK_HD bool decode_echo(const uint8_t* d, uint32_t len, Ctl& c) {
  if (len < 4) return false;
  c.id = be16(d);
  c.seq = be16(d + 2);
  return true;
}

// arp.go:42-67; NextLayerType is Payload (:106-108)
GPK_HD void decode_arp(const uint8_t* d, uint32_t len, Ctl& c) {
  if (len < 8) return fail(c, GPK_CTL_ERR_ARP_SHORT, len);
  const uint32_t hw = d[4], prot = d[5], arp_len = 8 + 2 * hw + 2 * prot;
  if (len < arp_len) return fail(c, GPK_CTL_ERR_ARP_EXPECTED, len, arp_len);
  c.addr_type = be16(d);
  c.protocol = be16(d + 2);
  c.hw = hw;
  c.prot = prot;
  c.op = be16(d + 6);
  done(c, arp_len, len, GPK_LT_PAYLOAD);
}

// The pseudo-header's network layer: the last one of the decoded list, from its
// layout slot. off: packet offset of SrcIP‖DstIP, bytes: their length (8 or 32);
// false: there is none (or its kind is dirty, P6)
struct Net {
  uint32_t off, bytes;
};
GPK_HD bool network_layer(uint32_t caplen, const gpk_record& rec, const gpk_layout& L, Net& net) {
  const uint32_t nl = (rec.status >> GPK_ST_NLAYERS_SHIFT) & GPK_ST_NLAYERS_MASK;
  for (uint32_t k = nl < GPK_MAX_INLINE_LAYERS ? nl : GPK_MAX_INLINE_LAYERS; k-- > 0;) {
    const uint32_t code = (uint32_t)(rec.layers >> (4 * k)) & 15u;
    if (code != GPK_CODE_IPV4 && code != GPK_CODE_IPV6) continue;
    const uint32_t s = L.start[code - 1], e = L.end[code - 1];
    const uint32_t from = code == GPK_CODE_IPV4 ? 12u : 8u, to = code == GPK_CODE_IPV4 ? 20u : 40u;
    if (s == GPK_LAYOUT_ABSENT || e > caplen || s > e || e - s < to) return false;
    net.off = s + from;
    net.bytes = to - from;
    return true;
  }
  return false;
}

// computeChecksum's start value (tcpip.go:54-69) from the sum of the address words
// (pseudoheaderChecksum, :26-48) and the message length
GPK_HD uint32_t start_value(uint32_t address_words, uint32_t length) {
  return address_words + 58u + (length & 0xffffu) + (length >> 16);
}

// One packet of gpk_control_batch: the class (GPK_CTL_CLASS_*), GPK_CTL_NONE or
// GPK_CTL_UNKNOWN; c is written for a class.
GPK_HD int control(const DevTables* T, uint32_t kinds, uint32_t flags, const uint8_t* p, uint32_t caplen,
                   const gpk_record& rec, const gpk_layout& L, Ctl& c) {
  static_assert(GPK_CTL_NONE == GPK_TUN_NONE && GPK_CTL_UNKNOWN == GPK_TUN_UNKNOWN, "tun::candidate's verdicts");
  tun::Pay pay;
  if (const int no = tun::candidate(T, p, caplen, rec, L, pay)) return no;
  const uint32_t k = kind_of_type(pay.next) & kinds;
  if (!k) return GPK_CTL_NONE;
  c = ctl_init(k, pay.off);
  const uint8_t* d = p + pay.off;
  int cls;
  if (k == GPK_CTL_ICMP4) {
    decode_icmp4(d, pay.len, c);
    c.lt0 = GPK_LT_ICMPV4;
    cls = GPK_CTL_CLASS_ICMP4;
  } else if (k == GPK_CTL_ICMP6) {
    decode_icmp6(d, pay.len, c);
    c.lt0 = GPK_LT_ICMPV6;
    cls = GPK_CTL_CLASS_ICMP6;
  } else if (k == GPK_CTL_ARP) {
    decode_arp(d, pay.len, c);
    c.lt0 = GPK_LT_ARP;
    cls = GPK_CTL_CLASS_ARP;
  } else {  // ICMPv6Echo in front, through a table edit
    if (!decode_echo(d, pay.len, c)) fail(c, GPK_CTL_ERR_ECHO_SHORT);
    else c.payload_off = pay.off, c.next = GPK_LT_PAYLOAD;
    c.lt0 = GPK_LT_ICMPV6_ECHO;
    cls = GPK_CTL_CLASS_ICMP6;
  }
  if (c.err) {
    c.lt0 = 0;
    return GPK_CTL_CLASS_FAILED;
  }
  c.nlayers = 1;
  // the loop goes on (layers_decoder.go:60-79): an empty payload ends it with nil
  if (c.payload_len) {
    if (c.next == GPK_LT_ICMPV6_ECHO && (kinds & GPK_CTL_ICMP6ECHO)) {
      if (decode_echo(p + c.payload_off, c.payload_len, c)) {
        c.lt1 = GPK_LT_ICMPV6_ECHO;  // its payload is empty: the loop ends here
        c.nlayers = 2;
      } else {
        c.err = GPK_CTL_ERR_ECHO_SHORT;
        c.status |= GPK_CTL_ST_TRUNCATED;
      }
    } else if (c.next == GPK_LT_PAYLOAD && T->dispatch[GPK_LT_PAYLOAD] == GPK_DEC_PAYLOAD) {
      c.lt1 = GPK_LT_PAYLOAD;  // base.go:61-70: never fails, no payload
      c.nlayers = 2;
    } else {
      c.unsupported = c.next;
    }
  }
  if ((flags & GPK_CTL_CSUM) && k == GPK_CTL_ICMP6) {  // the start value itself is the sum step's
    Net net;
    if (!network_layer(caplen, rec, L, net)) c.status |= GPK_CTL_ST_NONET;
  }
  return cls;
}

// the entries whose Contents‖Payload a sum covers: a decoded ICMPv4 / ICMPv6 header with a start value
GPK_HD bool wants_sum(uint32_t kind, uint32_t nlayers, uint32_t status) {
  return nlayers != 0 && (kind & (GPK_CTL_ICMP4 | GPK_CTL_ICMP6)) && !(status & GPK_CTL_ST_NONET);
}

// VerifyChecksum (icmp4.go:265-276, icmp6.go:263-277) from sum = ComputeChecksum(Contents‖Payload, start) mod 2^32
GPK_HD uint32_t correct_of(uint32_t sum, uint32_t existing) { return tun::fold16(sum - existing); }
GPK_HD uint32_t sum_status(uint32_t correct, uint32_t existing) {
  return GPK_CTL_ST_CSUM | (correct == existing ? GPK_CTL_ST_VALID : 0u);
}

}  // namespace ctl
}  // namespace gpk
