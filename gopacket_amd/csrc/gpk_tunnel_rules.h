// gpk_tunnel_rules.h — the per-packet rules of gpk_tunnel_batch, shared by the
// kernels and gpk_tunnel_batch_host (one __host__ __device__ source, so the CPU
// suite checks the code the device runs).
//
//   last_payload   LayerPayload() and NextLayerType() of the last layer of a
//                  decoded list, from its gpk_layout slot. The layer decoded
//                  without error (it is in the list), so only the success paths
//                  of layers/{ethernet,dot1q,ip4,ip6,tcp,udp}.go are restated;
//                  they mirror dec_* of gpk_device.h line by line.
//   candidate      whether a decoded list ends in a layer with a payload inside
//                  the packet, and last_payload of it (gpk_control_rules.h
//                  starts from it too)
//   decode_vxlan / decode_gre / decode_geneve
//                  DecodeFromBytes of layers/{vxlan,gre,geneve}.go with Go's
//                  bounds rules: data[i] needs i < len, data[:hi] needs hi <=
//                  cap, data[lo:] needs lo <= len.
#pragma once
#include <stdint.h>

#include "../../include/gpk_tunnel.h"
#include "gpk_device.h"

#define GPK_HD __host__ __device__ __forceinline__

namespace gpk {
namespace tun {

GPK_HD uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }
GPK_HD uint32_t be32(const uint8_t* p) { return be16(p) << 16 | be16(p + 2); }

struct Pay {
  uint32_t off, len;  // LayerPayload(), off relative to the packet
  int32_t next;       // NextLayerType()
};

GPK_HD int32_t port_type(const int32_t* tab, const uint8_t* h) {  // tcp.go:591-597, udp.go:114-119
  const int32_t lt = tab[be16(h + 2)];
  return lt == GPK_LT_PAYLOAD ? tab[be16(h)] : lt;
}

// record code of the decoded list -> decoder kind (0: none)
GPK_HD int kind_of_code(uint32_t code) {
  if (code >= GPK_CODE_ETHERNET && code <= GPK_CODE_IPV6) return (int)code;
  if (code >= GPK_CODE_IPV6_HOPBYHOP && code <= GPK_CODE_IPV6_DESTINATION) return GPK_DEC_IPV6_EXT;
  if (code == GPK_CODE_TCP) return GPK_DEC_TCP;
  if (code == GPK_CODE_UDP) return GPK_DEC_UDP;
  if (code == GPK_CODE_PAYLOAD) return GPK_DEC_PAYLOAD;
  if (code == GPK_CODE_FRAGMENT) return GPK_DEC_FRAGMENT;
  return GPK_DEC_NONE;
}

GPK_HD Pay last_payload(const DevTables* T, int kind, const uint8_t* p, uint32_t s, uint32_t e) {
  const uint8_t* h = p + s;
  uint32_t len = e - s;
  uint32_t ro = e, rl = 0;
  int32_t rn = 0;
  switch (kind) {
    case GPK_DEC_ETHERNET: {  // ethernet.go:42-63
      uint32_t et = be16(h + 12), plen = len - 14;
      if (et < 0x0600) {
        if (plen >= et) plen = et;
        et = 0;
      }
      ro = s + 14, rl = plen, rn = T->ethertype[et];
      break;
    }
    case GPK_DEC_DOT1Q:  // dot1q.go:30-41
      ro = s + 4, rl = len - 4, rn = T->ethertype[be16(h + 2)];
      break;
    case GPK_DEC_IPV4: {  // ip4.go:178-271
      uint32_t length = be16(h + 2);
      const uint32_t hl = (h[0] & 15u) * 4, ff = be16(h + 6);
      if (length == 0) length = len & 0xffff;
      if (len > length) len = length;
      ro = s + hl, rl = len - hl, rn = ((ff & 0x2000u) || (ff & 0x1fffu)) ? GPK_LT_FRAGMENT : T->ipprotocol[h[9]];
      break;
    }
    case GPK_DEC_IPV6: {  // ip6.go:221-278
      uint32_t length = be16(h + 4), nh = h[6], poff = s + 40, plen = len - 40, next_nh = nh;
      if (nh == 0) {
        const uint8_t* x = p + poff;
        const uint32_t hnh = x[0], actual = x[1] * 8u + 8u;
        bool have = false;
        uint32_t jl = 0;
        for (uint32_t q = 2; q < actual;) {  // the first jumbo TLV (ip6.go:54-76)
          const uint32_t t = x[q];
          uint32_t al = 1;
          if (t != 0) {
            al = x[q + 1] + 2u;
            if (t == 0xC2 && !have) {
              have = true;
              jl = be32(x + q + 2);
            }
          }
          q += al;
        }
        next_nh = hnh;
        if (have) {  // payload stays at the HopByHop header (ip6.go:249-256)
          ro = poff, rl = jl > plen ? plen : jl, rn = T->ipprotocol[hnh];
          break;
        }
        poff += actual;
        plen -= actual;
      }
      if (length > plen) length = plen;
      ro = poff, rl = length, rn = T->ipprotocol[next_nh];
      break;
    }
    case GPK_DEC_IPV6_EXT: {  // ip6.go:418-461
      const uint32_t actual = h[1] * 8u + 8u;
      ro = s + actual, rl = len - actual, rn = T->ipprotocol[h[0]];
      break;
    }
    case GPK_DEC_TCP: {  // tcp.go:291-551
      const uint32_t ds = (h[12] >> 4) * 4u;
      ro = s + ds, rl = len - ds, rn = port_type(T->tcp_port, h);
      break;
    }
    case GPK_DEC_UDP: {  // udp.go:30-56
      const uint32_t length = be16(h + 4);
      uint32_t hlen = len;
      if (length >= 8 && length <= len) hlen = length;
      ro = s + 8, rl = hlen - 8, rn = port_type(T->udp_port, h);
      break;
    }
    default:  // Payload / Fragment: no payload, next 0 (base.go:61-70, :115-124)
      break;
  }
  return Pay{ro, rl, rn};
}

// What a pass over a decoded batch looks at: the payload and next type of the
// list's last layer. 0: pay is set and lies inside caplen, not empty;
// GPK_TUN_UNKNOWN: the list is longer than the record names; GPK_TUN_NONE: a
// decode error, no layer with a payload, or a dirty layout slot.
GPK_HD int candidate(const DevTables* T, const uint8_t* p, uint32_t caplen, const gpk_record& rec, const gpk_layout& L,
                     Pay& pay) {
  const uint32_t nl = (rec.status >> GPK_ST_NLAYERS_SHIFT) & GPK_ST_NLAYERS_MASK;
  if (nl > GPK_MAX_INLINE_LAYERS) return GPK_TUN_UNKNOWN;
  const uint32_t err = rec.status & GPK_ST_ERR_MASK;
  if (nl == 0 || (err != GPK_ERR_NONE && err != GPK_ERR_UNSUPPORTED)) return GPK_TUN_NONE;
  const int kind = kind_of_code((uint32_t)(rec.layers >> (4 * (nl - 1))) & 15u);
  if (kind == GPK_DEC_NONE || kind >= GPK_DEC_PAYLOAD) return GPK_TUN_NONE;
  const uint32_t s = L.start[kind - 1], e = L.end[kind - 1];
  if (s == GPK_LAYOUT_ABSENT || e > caplen || s > e) return GPK_TUN_NONE;
  pay = last_payload(T, kind, p, s, e);
  if (pay.len == 0 || pay.off > caplen || pay.len > caplen - pay.off) return GPK_TUN_NONE;
  return 0;
}

GPK_HD uint32_t kind_of_type(int32_t lt) {
  return lt == GPK_LT_GRE ? GPK_TUN_GRE : lt == GPK_LT_VXLAN ? GPK_TUN_VXLAN : lt == GPK_LT_GENEVE ? GPK_TUN_GENEVE : 0u;
}

// A gpk_tunnel being decoded, one dword per field: the packed record's byte
// fields would put a lane's struct into scratch memory; this one stays in
// registers and is packed once, at the store.
struct Tun {
  uint32_t kind, err, status, bits, a0, a1, hdr_off, contents_len, inner_off, inner_len;
  int32_t next;
  uint32_t vni, protocol, gbp_id, raw0, raw1, checksum, offset, correct, key, seq, ack, count, list_off;
  uint32_t version, options_length;
};

GPK_HD Tun tun_init(uint32_t kind, uint32_t hdr_off) {
  Tun t;
  t.kind = kind;
  t.hdr_off = hdr_off;
  t.err = t.status = t.bits = t.a0 = t.a1 = t.contents_len = t.inner_off = t.inner_len = 0;
  t.next = 0;
  t.vni = t.protocol = t.gbp_id = t.raw0 = t.raw1 = t.checksum = t.offset = t.correct = t.key = t.seq = t.ack = 0;
  t.count = t.list_off = t.version = t.options_length = 0;
  return t;
}

// the packed record (include/gpk_tunnel.h), as 18 little-endian dwords
GPK_HD void tun_store(gpk_tunnel* dst, const Tun& t) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = t.kind | t.err << 8 | t.status << 16 | t.bits << 24;
  w[1] = t.a0;
  w[2] = t.a1;
  w[3] = t.hdr_off;
  w[4] = t.contents_len;
  w[5] = t.inner_off;
  w[6] = t.inner_len;
  w[7] = (uint32_t)t.next;
  w[8] = t.vni;
  w[9] = t.protocol | t.gbp_id << 16;
  w[10] = t.raw0 | t.raw1 << 8 | t.checksum << 16;
  w[11] = t.offset | t.correct << 16;
  w[12] = t.key;
  w[13] = t.seq;
  w[14] = t.ack;
  w[15] = t.count;
  w[16] = t.list_off;
  w[17] = t.version | t.options_length << 8;
}

GPK_HD void fail(Tun& t, uint32_t trunc, uint32_t code, uint32_t a0 = 0, uint32_t a1 = 0) {
  t = tun_init(t.kind, t.hdr_off);
  t.err = code;
  t.a0 = a0;
  t.a1 = a1;
  t.status = trunc ? GPK_TUN_ST_TRUNCATED : 0;
}

GPK_HD void done(Tun& t, uint32_t contents, uint32_t len, int32_t next) {
  t.contents_len = contents;
  t.inner_off = t.hdr_off + contents;
  t.inner_len = len - contents;
  t.next = next;
}

// vxlan.go:53-78; next is always Ethernet (:48-50)
GPK_HD void decode_vxlan(const uint8_t* d, uint32_t len, Tun& t) {
  if (len < 8) return fail(t, 0, GPK_TUN_ERR_VXLAN_SMALL);
  t.raw0 = d[0];
  t.raw1 = d[1];
  t.bits = (d[0] & 0x08 ? GPK_TUN_VX_I : 0) | (d[0] & 0x80 ? GPK_TUN_VX_G : 0) | (d[1] & 0x40 ? GPK_TUN_VX_D : 0) |
           (d[1] & 0x80 ? GPK_TUN_VX_A : 0);
  t.gbp_id = be16(d + 2);
  t.vni = (uint32_t)d[4] << 16 | (uint32_t)d[5] << 8 | d[6];
  done(t, 8, len, GPK_LT_ETHERNET);
}

// gre.go:40-128; every slice is guarded by requireBytes, so no panic exists
GPK_HD void decode_gre(const DevTables* T, const uint8_t* d, uint32_t len, Tun& t) {
  if (len < 4) return fail(t, 1, GPK_TUN_ERR_GRE_SMALL);
  const uint32_t b0 = d[0], b1 = d[1];
  t.raw0 = b0;
  t.raw1 = b1;
  t.protocol = be16(d + 2);
  uint32_t off = 4;
  if (b0 & 0xC0) {  // ChecksumPresent || RoutingPresent
    if (len - off < 4) return fail(t, 1, GPK_TUN_ERR_GRE_TRUNCATED);
    t.checksum = be16(d + off);
    t.offset = be16(d + off + 2);
    off += 4;
  }
  if (b0 & 0x20) {
    if (len - off < 4) return fail(t, 1, GPK_TUN_ERR_GRE_TRUNCATED);
    t.key = be32(d + off);
    off += 4;
  }
  if (b0 & 0x10) {
    if (len - off < 4) return fail(t, 1, GPK_TUN_ERR_GRE_TRUNCATED);
    t.seq = be32(d + off);
    off += 4;
  }
  if (b0 & 0x40) {
    t.list_off = t.hdr_off + off;
    uint32_t listed = 0;
    for (;;) {
      if (len - off < 4) return fail(t, 1, GPK_TUN_ERR_GRE_TRUNCATED);
      const uint32_t af = be16(d + off), sl = d[off + 3];
      if (len - (off + 4) < sl) return fail(t, 1, GPK_TUN_ERR_GRE_TRUNCATED);
      off += 4 + sl;
      if (af == 0 && sl == 0) break;
      listed++;
    }
    t.count = listed;
  }
  if (b1 & 0x80) {
    if (len - off < 4) return fail(t, 1, GPK_TUN_ERR_GRE_TRUNCATED);
    t.ack = be32(d + off);
    off += 4;
  }
  done(t, off, len, T->ethertype[t.protocol]);
}

// geneve.go:59-119
GPK_HD void decode_geneve(const DevTables* T, const uint8_t* d, uint32_t len, uint32_t cap, Tun& t) {
  if (len < 7) return fail(t, 1, GPK_TUN_ERR_GENEVE_SHORT);
  t.raw0 = d[0];
  t.raw1 = d[1];
  t.version = d[0] >> 7;
  t.options_length = (d[0] & 0x3fu) * 4;
  t.bits = (d[1] & 0x80 ? GPK_TUN_GN_O : 0) | (d[1] & 0x40 ? GPK_TUN_GN_C : 0);
  t.protocol = be16(d + 2);
  t.vni = (uint32_t)d[4] << 16 | (uint32_t)d[5] << 8 | d[6];
  uint32_t offset = 8;  // uint8
  int32_t length = (int32_t)t.options_length;
  if (len < (uint32_t)length + 7) return fail(t, 1, GPK_TUN_ERR_GENEVE_OPTS_SHORT);
  t.list_off = t.hdr_off + 8;
  uint32_t n = 0;
  while (length > 0) {
    if (offset > len) return fail(t, 0, GPK_ERR_PANIC_SLICE_B, offset, len);  // data[offset:]
    const uint32_t left = len - offset;
    if (left < 3) return fail(t, 1, GPK_TUN_ERR_GENEVE_OPT_SHORT);
    if (left == 3) return fail(t, 0, GPK_ERR_PANIC_INDEX, 3, 3);  // data[3] after the len < 3 check
    const uint32_t ol = (d[offset + 3] & 0x1fu) * 4 + 4;
    if (left < ol) return fail(t, 1, GPK_TUN_ERR_GENEVE_OPT_LEN);
    n++;
    length -= (int32_t)ol;
    offset = (offset + ol) & 0xffu;
  }
  if (offset > cap) return fail(t, 0, GPK_ERR_PANIC_SLICE_ACAP, offset, cap);  // data[:offset]
  if (offset > len) return fail(t, 0, GPK_ERR_PANIC_SLICE_B, offset, len);     // data[offset:]
  t.count = n;
  done(t, offset, len, T->ethertype[t.protocol]);
}

// One packet of gpk_tunnel_batch: the class (GPK_TUN_CLASS_*), GPK_TUN_NONE or
// GPK_TUN_UNKNOWN; t is written for a class.
GPK_HD int peel(const DevTables* T, uint32_t kinds, const uint8_t* p, uint32_t caplen, const gpk_record& rec,
                const gpk_layout& L, Tun& t) {
  Pay pay;
  if (const int no = candidate(T, p, caplen, rec, L, pay)) return no;
  const uint32_t tk = kind_of_type(pay.next) & kinds;
  if (!tk) return GPK_TUN_NONE;
  t = tun_init(tk, pay.off);
  const uint8_t* d = p + pay.off;
  if (tk == GPK_TUN_VXLAN) decode_vxlan(d, pay.len, t);
  else if (tk == GPK_TUN_GRE) decode_gre(T, d, pay.len, t);
  else decode_geneve(T, d, pay.len, caplen - pay.off, t);
  if (t.err) return GPK_TUN_CLASS_FAILED;
  if (t.inner_len == 0 || t.next < 0 || t.next >= GPK_MAX_LAYER_TYPE) return GPK_TUN_CLASS_NOINNER;
  switch (T->dispatch[t.next]) {
    case GPK_DEC_ETHERNET: return GPK_TUN_CLASS_ETHERNET;
    case GPK_DEC_DOT1Q: return GPK_TUN_CLASS_DOT1Q;
    case GPK_DEC_IPV4: return GPK_TUN_CLASS_IPV4;
    case GPK_DEC_IPV6: return GPK_TUN_CLASS_IPV6;
    default: return GPK_TUN_CLASS_NOINNER;
  }
}

// the entries whose Contents‖Payload the GRE sum covers: a decoded GRE header with the C bit
GPK_HD bool wants_sum(const Tun& t) { return t.kind == GPK_TUN_GRE && !t.err && (t.raw0 & 0x80); }

// checksum.go:53-58
GPK_HD uint32_t fold16(uint32_t c) {
  c = (c >> 16) + (c & 0xffff);
  c = (c >> 16) + (c & 0xffff);
  return (~c) & 0xffff;
}

// GRE.VerifyChecksum (gre.go:239-250) from sum = ComputeChecksum(Contents‖Payload, 0) mod 2^32:
// Correct, and the status bits it adds
GPK_HD uint32_t gre_correct(uint32_t sum, uint32_t existing) { return fold16(sum - existing); }
GPK_HD uint32_t gre_status(uint32_t correct, uint32_t existing) {
  return GPK_TUN_ST_CSUM | (correct == existing ? GPK_TUN_ST_VALID : 0u);
}

}  // namespace tun
}  // namespace gpk
