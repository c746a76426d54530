// gpk_svc_rules.h — the per-message rules of gpk_svc_batch, shared by the
// kernels and gpk_svc_batch_host (one __host__ __device__ source, so the CPU
// suite checks the code the device runs).
//
//   dhcp4_options<kEmit>  the loop of DHCPv4.DecodeFromBytes over
//                         DHCPOption.decode (dhcpv4.go:160-179, 563-583)
//   dhcp6_options<kEmit>  the loop of DHCPv6.DecodeFromBytes over
//                         DHCPv6Option.decode (dhcpv6.go:113-121,
//                         dhcpv6_options.go:611-622), the uint16 sum included
//   walk<kEmit>           DecodeFromBytes of the three layers (dhcpv4.go:126-184,
//                         dhcpv6.go:89-124, ntp.go:294-347) in two forms of one
//                         function: counting (class, error, nentries, the
//                         scalars) and emit (the gpk_svc_entry descriptors too)
//   svc                   one packet: tun::candidate, then walk<false>
// The lane's state is scalars only: no array is indexed at run time.
#pragma once
#include <stdint.h>

#include "../../include/gpk_svc.h"
#include "gpk_tunnel_rules.h"

namespace gpk {
namespace svc {

using tun::be16;
using tun::be32;

GPK_HD uint32_t kind_of_type(int32_t lt) {
  switch (lt) {
    case GPK_LT_DHCPV4: return GPK_SVC_DHCP4;
    case GPK_LT_DHCPV6: return GPK_SVC_DHCP6;
    case GPK_LT_NTP: return GPK_SVC_NTP;
    default: return 0u;
  }
}

// A gpk_svc being decoded, one dword per field (as ndp::Msg): it stays in
// registers and is packed once, at the store.
struct Msg {
  uint32_t lt, err, a0, a1, status, hdr_off, len, contents_len, nentries, b, v0, v1, v2, v3, v4, v5;
};

GPK_HD void msg_init(Msg& m, uint32_t lt, uint32_t hdr_off) {
  m.lt = lt;
  m.hdr_off = hdr_off;
  m.err = m.a0 = m.a1 = m.status = m.len = m.contents_len = m.nentries = m.b = 0;
  m.v0 = m.v1 = m.v2 = m.v3 = m.v4 = m.v5 = 0;
}

// the packed record (include/gpk_svc.h) as 16 little-endian dwords; entry0 is the emit step's
GPK_HD void msg_store(gpk_svc* dst, const Msg& m) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = m.lt | m.err << 8 | m.status << 16;
  w[1] = m.a0;
  w[2] = m.a1;
  w[3] = m.hdr_off;
  w[4] = m.len;
  w[5] = m.contents_len;
  w[6] = w[7] = 0;
  w[8] = m.nentries;
  w[9] = m.b;
  w[10] = m.v0, w[11] = m.v1, w[12] = m.v2, w[13] = m.v3, w[14] = m.v4, w[15] = m.v5;
}

GPK_HD void entry_store(gpk_svc_entry* dst, uint32_t code, uint32_t length, uint32_t off) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = code | length << 16;
  w[1] = off;
}

// four packet bytes in packet order, as the dword a little-endian store puts back in that order
GPK_HD uint32_t le32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

// What an option loop found: its error (0: none) with the two arguments, and
// the options in front of it. Built from locals at one return, and walk below
// stores a Msg once, from locals, on every path alike: stores to different
// fields on different paths are what the compiler turns into an indexed store
// to a struct in scratch.
struct Opts {
  uint32_t err, a0, a1, k;
};

// dhcpv4.go:160-179 over d[240:len] (len > 240); option k of the message goes to out[k] when kEmit
template <bool kEmit>
GPK_HD Opts dhcp4_options(const uint8_t* d, uint32_t len, uint32_t at, gpk_svc_entry* out) {
  uint32_t off = 240, k = 0, err = 0;
  while (off < len) {
    const uint32_t type = d[off];
    if (type == 255) break;  // End: not appended, the rest is ignored
    uint32_t length = 0, step = 1;  // Pad: one byte, appended
    if (type != 0) {
      const uint32_t left = len - off;  // >= 1
      if (left < 2) {
        err = GPK_SVC_ERR_DHCP4_OPT_SHORT;
        break;
      }
      length = d[off + 1];
      if (length > left - 2) {
        err = GPK_SVC_ERR_DHCP4_OPT_MALFORMED;
        break;
      }
      step = 2;
    }
    if (kEmit) entry_store(out + k, type, length, at + off + step);
    k++;
    off += step + length;
  }
  return Opts{err, 0, 0, k};
}

// dhcpv6.go:113-121 over d[off:len] with dhcpv6_options.go:611-622 per option
template <bool kEmit>
GPK_HD Opts dhcp6_options(const uint8_t* d, uint32_t len, uint32_t off, uint32_t at, gpk_svc_entry* out) {
  uint32_t k = 0, err = 0, a0 = 0, a1 = 0;
  while (off < len) {
    const uint32_t left = len - off;
    if (left < 4) {
      err = GPK_SVC_ERR_DHCP6_OPT_SHORT;
      break;
    }
    const uint32_t length = be16(d + off + 2), end16 = (4 + length) & 0xFFFFu;  // 4 + o.Length in uint16
    if (left < 4 + length) {
      err = GPK_SVC_ERR_DHCP6_OPT_LENGTH, a0 = end16;
      break;
    }
    if (end16 < 4) {  // data[4 : 4+o.Length]: the high bound wrapped below the low one
      err = GPK_ERR_PANIC_SLICE_B, a0 = 4, a1 = end16;
      break;
    }
    if (kEmit) entry_store(out + k, be16(d + off), length, at + off + 4);
    k++;
    off += 4 + length;
  }
  return Opts{err, a0, a1, k};
}

GPK_HD uint32_t truncated(uint32_t err) {
  return err == GPK_SVC_ERR_DHCP4_SHORT || err == GPK_SVC_ERR_DHCP6_SHORT || err == GPK_SVC_ERR_DHCP6_RELAY_SHORT ||
                 err == GPK_SVC_ERR_NTP_SHORT
             ? GPK_SVC_ST_TRUNCATED
             : 0u;
}

// DecodeFromBytes(d[:len]) of the layer m.lt at m.hdr_off; m's other fields
// are written, a failed message's as 0. kEmit: entry k of the message goes to
// out[k] (the caller has checked that the range fits).
template <bool kEmit>
GPK_HD void walk(const uint8_t* d, uint32_t len, Msg& m, gpk_svc_entry* out) {
  const uint32_t at = m.hdr_off, lt = m.lt;
  uint32_t clen = len, b = 0, v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0;
  Opts o{0, 0, 0, 0};
  if (lt == GPK_LT_DHCPV4) {  // dhcpv4.go:126-184
    if (len < 240) o.err = GPK_SVC_ERR_DHCP4_SHORT, o.a0 = len;
    else if (d[2] > 16) o.err = GPK_SVC_ERR_DHCP4_HLEN, o.a0 = d[2];
    else if (be32(d + 236) != 0x63825363u) o.err = GPK_SVC_ERR_DHCP4_MAGIC;
    else {
      b = le32(d);
      v0 = be32(d + 4);
      v1 = be16(d + 8) | be16(d + 10) << 16;
      v2 = le32(d + 12), v3 = le32(d + 16), v4 = le32(d + 20), v5 = le32(d + 24);
      if (len == 240) clen = 0;  // :155-158: no options, and Contents stays unset
      else o = dhcp4_options<kEmit>(d, len, at, out);
    }
  } else if (lt == GPK_LT_DHCPV6) {  // dhcpv6.go:89-124
    const uint32_t type = len ? d[0] : 0u;
    const bool relay = type == 12 || type == 13;
    if (len < 4) o.err = GPK_SVC_ERR_DHCP6_SHORT, o.a0 = len;
    else if (relay && len < 34) o.err = GPK_SVC_ERR_DHCP6_RELAY_SHORT, o.a0 = len, o.a1 = type;
    else {
      b = relay ? type | (uint32_t)d[1] << 8 : type;
      v0 = relay ? 0u : (uint32_t)d[1] << 16 | d[2] << 8 | d[3];
      v1 = relay ? at + 2 : 0u;
      v2 = relay ? at + 18 : 0u;
      o = dhcp6_options<kEmit>(d, len, relay ? 34 : 4, at, out);
    }
  } else {  // GPK_LT_NTP, ntp.go:294-347
    if (len < 48) o.err = GPK_SVC_ERR_NTP_SHORT;
    else {
      b = (uint32_t)d[0] >> 6 | ((d[0] >> 3) & 7u) << 8 | (d[0] & 7u) << 16 | (uint32_t)d[1] << 24;
      v0 = d[2] | d[3] << 8;
      v1 = be32(d + 4);
      v2 = be32(d + 8);
      v3 = be32(d + 12);
      v4 = at + 48;
      v5 = len - 48;
    }
  }
  const uint32_t keep = o.err ? 0u : ~0u;  // a failed message keeps its type, error and offset only
  m.err = o.err, m.a0 = o.a0, m.a1 = o.a1;
  m.status = truncated(o.err);
  m.len = len & keep, m.contents_len = clen & keep, m.nentries = o.k & keep, m.b = b & keep;
  m.v0 = v0 & keep, m.v1 = v1 & keep, m.v2 = v2 & keep, m.v3 = v3 & keep, m.v4 = v4 & keep, m.v5 = v5 & keep;
}

// One packet of gpk_svc_batch: the class (GPK_SVC_CLASS_*), GPK_SVC_NONE or
// GPK_SVC_UNKNOWN; m is written for a class.
GPK_HD int svc(const DevTables* T, uint32_t kinds, const uint8_t* p, uint32_t caplen, const gpk_record& rec,
               const gpk_layout& L, Msg& m) {
  static_assert(GPK_SVC_NONE == GPK_TUN_NONE && GPK_SVC_UNKNOWN == GPK_TUN_UNKNOWN, "tun::candidate's verdicts");
  tun::Pay pay;
  if (const int no = tun::candidate(T, p, caplen, rec, L, pay)) return no;
  if (!(kind_of_type(pay.next) & kinds)) return GPK_SVC_NONE;
  msg_init(m, (uint32_t)pay.next, pay.off);
  walk<false>(p + pay.off, pay.len, m, nullptr);
  return m.err ? GPK_SVC_CLASS_FAILED : GPK_SVC_CLASS_OK;
}

}  // namespace svc
}  // namespace gpk
