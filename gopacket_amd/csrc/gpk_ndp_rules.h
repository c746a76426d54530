// gpk_ndp_rules.h — the per-message rules of gpk_ndp_batch, shared by the
// kernels and gpk_ndp_batch_host (one __host__ __device__ source, so the CPU
// suite checks the code the device runs).
//
//   options<kEmit>  ICMPv6Options.DecodeFromBytes (icmp6msg.go:514-546)
//   records<kEmit>  the loop of MLDv2MulticastListenerReportMessage over
//                   MLDv2MulticastAddressRecord.decode (mldv2.go:309-333, 473-509)
//   walk<kEmit>     DecodeFromBytes of the ten layers in two forms of one
//                   function: counting (class, error, nentries, the scalars)
//                   and emit (the gpk_ndp_entry descriptors as well)
//   ndp             one packet: tun::candidate, the two ways in (behind
//                   ctl::decode_icmp6 / ctl::icmp6_next, or in front through a
//                   table edit), then walk<false>
// The lane's state is scalars only: no array is indexed at run time.
#pragma once
#include <stdint.h>

#include "../../include/gpk_ndp.h"
#include "gpk_control_rules.h"

namespace gpk {
namespace ndp {

using tun::be16;
using tun::be32;

GPK_HD uint32_t kind_of_type(int32_t lt) {
  switch (lt) {
    case GPK_LT_ICMPV6_ROUTER_SOLICITATION: return GPK_NDP_RS;
    case GPK_LT_ICMPV6_ROUTER_ADVERTISEMENT: return GPK_NDP_RA;
    case GPK_LT_ICMPV6_NEIGHBOR_SOLICITATION: return GPK_NDP_NS;
    case GPK_LT_ICMPV6_NEIGHBOR_ADVERTISEMENT: return GPK_NDP_NA;
    case GPK_LT_ICMPV6_REDIRECT: return GPK_NDP_REDIRECT;
    case GPK_LT_MLDV1_QUERY: return GPK_NDP_MLD1_QUERY;
    case GPK_LT_MLDV1_REPORT: return GPK_NDP_MLD1_REPORT;
    case GPK_LT_MLDV1_DONE: return GPK_NDP_MLD1_DONE;
    case GPK_LT_MLDV2_QUERY: return GPK_NDP_MLD2_QUERY;
    case GPK_LT_MLDV2_REPORT: return GPK_NDP_MLD2_REPORT;
    default: return 0u;
  }
}

// A gpk_ndp being decoded, one dword per field (as ctl::Ctl): it stays in
// registers and is packed once, at the store.
struct Msg {
  uint32_t lt, err, a0, a1, status, flags, hdr_off, len, contents_len, payload_off, payload_len;
  uint32_t v0, v1, v2, v3, nentries, count, s_qrv, qqic;
};

GPK_HD void msg_init(Msg& m, uint32_t lt, uint32_t hdr_off) {
  m.lt = lt;
  m.hdr_off = hdr_off;
  m.err = m.a0 = m.a1 = m.status = m.flags = m.len = m.contents_len = m.payload_off = m.payload_len = 0;
  m.v0 = m.v1 = m.v2 = m.v3 = m.nentries = m.count = m.s_qrv = m.qqic = 0;
}

// the packed record (include/gpk_ndp.h) as 16 little-endian dwords; entry0 is the emit step's
GPK_HD void msg_store(gpk_ndp* dst, const Msg& m) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = m.lt | m.err << 8 | m.status << 16 | m.flags << 24;
  w[1] = m.a0;
  w[2] = m.a1;
  w[3] = m.hdr_off;
  w[4] = m.len;
  w[5] = m.contents_len;
  w[6] = m.payload_off;
  w[7] = m.payload_len;
  w[8] = m.v0, w[9] = m.v1, w[10] = m.v2, w[11] = m.v3;
  w[12] = w[13] = 0;
  w[14] = m.nentries;
  w[15] = m.count | m.s_qrv << 16 | m.qqic << 24;
}

GPK_HD void entry_store(gpk_ndp_entry* dst, uint32_t type, uint32_t aux, uint32_t n, uint32_t off, uint32_t ext,
                        uint32_t aux_off) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = type | aux << 8 | n << 16;
  w[1] = off;
  w[2] = ext;
  w[3] = aux_off;
}

GPK_HD void fail(Msg& m, uint32_t code, uint32_t a0 = 0, uint32_t a1 = 0) {
  msg_init(m, m.lt, m.hdr_off);
  m.err = code;
  m.a0 = a0;
  m.a1 = a1;
  m.status = code == GPK_NDP_ERR_RECORD_AUX ? 0u : GPK_NDP_ST_TRUNCATED;
}

// ICMPv6Options.DecodeFromBytes(d[off:len]); option k of the message goes to out[k] when kEmit
template <bool kEmit>
GPK_HD void options(const uint8_t* d, uint32_t len, uint32_t off, Msg& m, gpk_ndp_entry* out) {
  uint32_t k = 0;
  while (off < len) {
    const uint32_t left = len - off;
    if (left < 2) return fail(m, GPK_NDP_ERR_OPT_SHORT);
    const uint32_t length = d[off + 1] * 8u;
    if (length == 0) return fail(m, GPK_NDP_ERR_OPT_ZERO);
    if (left < length) return fail(m, GPK_NDP_ERR_OPT_OVERRUN, left, length);
    if (kEmit) entry_store(out + k, d[off], 0, 0, m.hdr_off + off + 2, length - 2, 0);
    k++;
    off += length;
  }
  m.nentries = k;
}

// mldv2.go:319-330 over d[4:len] with :473-509 per record; the sources are
// checked in one step: the first one whose end passes the data fails
template <bool kEmit>
GPK_HD void records(const uint8_t* d, uint32_t len, Msg& m, gpk_ndp_entry* out) {
  uint32_t begin = 4;
  for (uint32_t i = 0; i < m.count; i++) {
    const uint32_t left = len - begin;  // begin <= len: a record's length never exceeds what it was handed
    if (left < 20) return fail(m, GPK_NDP_ERR_RECORD_SHORT);
    const uint8_t* r = d + begin;
    const uint32_t aux = r[1], n = be16(r + 2), fits = (left - 20) / 16;
    if (n > fits) return fail(m, GPK_NDP_ERR_RECORD_SOURCES, 20 + 16 * (fits + 1));
    const uint32_t without = 20 + 16 * n, total = without + 4 * aux;
    if (left < total) return fail(m, GPK_NDP_ERR_RECORD_AUX, without);
    const uint32_t at = m.hdr_off + begin;
    if (kEmit) entry_store(out + i, r[0], aux, n, at + 4, at + 20, at + without);
    begin += total;
  }
  m.nentries = m.count;
}

// DecodeFromBytes(d[:len]) of the layer m.lt. kEmit: entry k of the message
// goes to out[k] (the caller has checked that the range fits).
template <bool kEmit>
GPK_HD void walk(const uint8_t* d, uint32_t len, Msg& m, gpk_ndp_entry* out) {
  const uint32_t at = m.hdr_off;
  switch (m.lt) {
    case GPK_LT_ICMPV6_ROUTER_SOLICITATION:  // icmp6msg.go:190-202: no BaseLayer
      if (len < 4) return fail(m, GPK_NDP_ERR_RS_SHORT);
      m.len = len;
      return options<kEmit>(d, len, 4, m, out);
    case GPK_LT_ICMPV6_ROUTER_ADVERTISEMENT:  // :237-255
      if (len < 12) return fail(m, GPK_NDP_ERR_RA_SHORT);
      m.len = m.contents_len = len;
      m.v3 = d[0];
      m.flags = d[1];
      m.v2 = be16(d + 2);
      m.v0 = be32(d + 4);
      m.v1 = be32(d + 8);
      return options<kEmit>(d, len, 12, m, out);
    case GPK_LT_ICMPV6_NEIGHBOR_SOLICITATION:  // :306-319
      if (len < 20) return fail(m, GPK_NDP_ERR_NS_SHORT);
      m.len = m.contents_len = len;
      m.v0 = at + 4;
      return options<kEmit>(d, len, 20, m, out);
    case GPK_LT_ICMPV6_NEIGHBOR_ADVERTISEMENT:  // :355-369
      if (len < 20) return fail(m, GPK_NDP_ERR_NA_SHORT);
      m.len = m.contents_len = len;
      m.flags = d[0];
      m.v0 = at + 4;
      return options<kEmit>(d, len, 20, m, out);
    case GPK_LT_ICMPV6_REDIRECT:  // :422-436
      if (len < 36) return fail(m, GPK_NDP_ERR_REDIRECT_SHORT);
      m.len = m.contents_len = len;
      m.v0 = at + 4;
      m.v1 = at + 20;
      return options<kEmit>(d, len, 36, m, out);
    case GPK_LT_MLDV1_QUERY:
    case GPK_LT_MLDV1_REPORT:
    case GPK_LT_MLDV1_DONE:  // mldv1.go:32-43: no BaseLayer; the query's Payload, :95-106
      if (len < 20) return fail(m, GPK_NDP_ERR_MLD1_SHORT);
      m.len = len;
      m.v2 = be16(d);
      m.v0 = at + 4;
      if (m.lt == GPK_LT_MLDV1_QUERY && len > 20) m.payload_off = at + 20, m.payload_len = len - 20;
      return;
    case GPK_LT_MLDV2_QUERY: {  // mldv2.go:61-90: the first source whose end passes the data fails
      if (len < 24) return fail(m, GPK_NDP_ERR_MLD2_QUERY_SHORT);
      const uint32_t n = be16(d + 22), fits = (len - 24) / 16;
      if (n > fits) return fail(m, GPK_NDP_ERR_MLD2_QUERY_SOURCES, 24 + 16 * (fits + 1));
      m.len = len;
      m.v2 = be16(d);
      m.v0 = at + 4;
      m.s_qrv = d[20] & 0xFu;
      m.qqic = d[21];
      m.count = n;
      return;
    }
    default:  // GPK_LT_MLDV2_REPORT, :309-333
      if (len < 4) return fail(m, GPK_NDP_ERR_MLD2_REPORT_SHORT);
      m.len = len;
      m.count = be16(d + 2);
      return records<kEmit>(d, len, m, out);
  }
}

// One packet of gpk_ndp_batch: the class (GPK_NDP_CLASS_*), GPK_NDP_NONE or
// GPK_NDP_UNKNOWN; m is written for a class.
GPK_HD int ndp(const DevTables* T, uint32_t kinds, const uint8_t* p, uint32_t caplen, const gpk_record& rec,
               const gpk_layout& L, Msg& m) {
  static_assert(GPK_NDP_NONE == GPK_TUN_NONE && GPK_NDP_UNKNOWN == GPK_TUN_UNKNOWN, "tun::candidate's verdicts");
  tun::Pay pay;
  if (const int no = tun::candidate(T, p, caplen, rec, L, pay)) return no;
  int32_t lt = pay.next;
  uint32_t off = pay.off, len = pay.len;
  if (lt == GPK_LT_ICMPV6) {  // way 1: behind the header the caller's layers.ICMPv6 decodes
    if (!(kinds & GPK_NDP_ICMP6)) return GPK_NDP_NONE;
    ctl::Ctl c = ctl::ctl_init(GPK_CTL_ICMP6, pay.off);
    ctl::decode_icmp6(p + pay.off, pay.len, c);
    if (c.err || c.payload_len == 0) return GPK_NDP_NONE;
    lt = c.next;
    off = c.payload_off;
    len = c.payload_len;
  }
  if (!(kind_of_type(lt) & kinds)) return GPK_NDP_NONE;
  msg_init(m, (uint32_t)lt, off);
  walk<false>(p + off, len, m, nullptr);
  return m.err ? GPK_NDP_CLASS_FAILED : GPK_NDP_CLASS_OK;
}

}  // namespace ndp
}  // namespace gpk
