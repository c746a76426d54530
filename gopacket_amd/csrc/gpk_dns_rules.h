// gpk_dns_rules.h — the per-message rules of gpk_dns_batch, shared by the
// kernels and gpk_dns_batch_host (one __host__ __device__ source, so the CPU
// suite checks the code the device runs).
//
//   decode_name    decodeName (dns.go:814-920) restated as a loop over levels: a
//                  pointer ends its level, so the recursion is a tail call
//   rdata          decodeRData (dns.go:1350-1529) over data[:end]
//   walk<kEmit>    DNS.DecodeFromBytes (dns.go:333-421) in two modes of one
//                  function: size only (class, error, nrr, name_bytes, the
//                  header fields), and emit (the gpk_dns_rr entries and the
//                  name bytes as well)
//   dns            one packet: tun::candidate, then walk<false>
// The functions that read bytes take them as B: a const uint8_t*, or a Seam
// (gpk_seam.h) for the one message of a stream that straddles the carried tail
// and the new bytes (gpk_dns_streams.hip).
// The lane's state is scalars only: no array is indexed at run time.
#pragma once
#include <stdint.h>

#include "../../include/gpk_dns.h"
#include "gpk_seam.h"
#include "gpk_tunnel_rules.h"

namespace gpk {
namespace dns {

using tun::be16;
using tun::be32;

// A gpk_dns being decoded, one dword per field (as ctl::Ctl)
struct Msg {
  uint32_t err, a0, a1, status, hdr_off, len, id, flags2, flags3, rcode, qd, an, ns, ar, nrr;
  uint64_t name_bytes;
};

GPK_HD void msg_init(Msg& m, uint32_t hdr_off) {
  m.err = m.a0 = m.a1 = m.status = m.len = m.id = m.flags2 = m.flags3 = m.rcode = 0;
  m.qd = m.an = m.ns = m.ar = m.nrr = 0;
  m.hdr_off = hdr_off;
  m.name_bytes = 0;
}

// the packed record (include/gpk_dns.h) as 16 little-endian dwords; rr0 and name0 are the emit step's
GPK_HD void msg_store(gpk_dns* dst, const Msg& m) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = GPK_DNS_KIND | m.err << 8 | m.status << 16 | m.rcode << 24;
  w[1] = m.a0;
  w[2] = m.a1;
  w[3] = m.hdr_off;
  w[4] = m.len;
  w[5] = m.id | m.flags2 << 16 | m.flags3 << 24;
  w[6] = m.qd | m.an << 16;
  w[7] = m.ns | m.ar << 16;
  w[8] = m.nrr;
  w[9] = 0;
  w[10] = w[11] = w[12] = w[13] = 0;
  w[14] = (uint32_t)m.name_bytes;
  w[15] = (uint32_t)(m.name_bytes >> 32);
}

// where the names go (emit mode) and the arguments of an error text
struct Cur {
  uint8_t* names;   // the arena
  uint64_t pos;     // the next name's place in it
  uint32_t a0, a1;
};

// decodeName(data[:len], offset, buffer, 1). The name's bytes go to c.names +
// c.pos when kEmit; n: its length; end: the returned offset (the top level's).
template <bool kEmit, typename B>
GPK_HD uint32_t decode_name(const B& d, uint32_t len, uint32_t offset, Cur& c, uint32_t& n, uint32_t& end) {
  uint8_t* out = kEmit ? c.names + c.pos : nullptr;
  uint32_t off = offset;
  n = 0;
  end = 0;
  for (uint32_t level = 1;; level++) {
    if (level > 255) return GPK_DNS_ERR_MAX_RECURSION;  // :815
    if (off >= len) return GPK_DNS_ERR_OFFSET_HIGH;     // :817
    uint32_t idx = off, next = 0;
    bool pointer = false;
    while (d[idx] != 0) {  // a first zero byte: the immediate return of :825-827, index + 1 as below
      const uint32_t b = d[idx], form = b & 0xc0u;
      if (form == 0) {  // :840-854
        const uint32_t idx2 = idx + b + 1;
        if (idx2 - off > 255) return GPK_DNS_ERR_NAME_LONG;
        if (idx2 > len) return GPK_DNS_ERR_INVALID_INDEX;
        if (kEmit) {
          if (n) out[n] = '.';
          uint8_t* o = out + n + (n ? 1 : 0);
          for (uint32_t k = 0; k < b; k++) o[k] = d[idx + 1 + k];
        }
        n += b + (n ? 1 : 0);  // the buffer's leading '.' is stripped (:919)
        idx = idx2;
      } else if (form == 0xc0u) {  // :876-902
        if (idx + 2 > len) return GPK_DNS_ERR_POINTER_HIGH;
        next = be16(d + idx) & 0x3fffu;
        if (next > len) return GPK_DNS_ERR_POINTER_HIGH;
        pointer = true;
        idx++;  // the pointer is two bytes
        break;
      } else {  // :904-910
        c.a0 = b;
        c.a1 = idx;
        return form == 0x40u ? GPK_DNS_ERR_QNAME40 : GPK_DNS_ERR_QNAME80;
      }
      if (idx >= len) return GPK_DNS_ERR_INDEX_RANGE;  // :912
    }
    if (level == 1) end = idx + 1;
    if (!pointer) return 0;
    off = next;
  }
}

// A gpk_dns_rr being decoded
struct Rr {
  uint32_t section, type, cls, data_length, ttl, data_off, name_len, count, rname_len, rname2_len;
  uint32_t v0, v1, v2, v3, v4, v5, v6, v7, v8, v9;
  uint64_t name_off, rname_off, rname2_off;
};

GPK_HD void rr_init(Rr& r, uint32_t section) {
  r.section = section;
  r.type = r.cls = r.data_length = r.ttl = r.data_off = r.name_len = r.count = r.rname_len = r.rname2_len = 0;
  r.v0 = r.v1 = r.v2 = r.v3 = r.v4 = r.v5 = r.v6 = r.v7 = r.v8 = r.v9 = 0;
  r.name_off = r.rname_off = r.rname2_off = 0;
}

GPK_HD void rr_store(gpk_dns_rr* dst, const Rr& r) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = r.section | r.type << 16;
  w[1] = r.cls | r.data_length << 16;
  w[2] = r.ttl;
  w[3] = r.data_off;
  w[4] = (uint32_t)r.name_off;
  w[5] = (uint32_t)(r.name_off >> 32);
  w[6] = r.name_len;
  w[7] = r.count;
  w[8] = (uint32_t)r.rname_off;
  w[9] = (uint32_t)(r.rname_off >> 32);
  w[10] = r.rname_len;
  w[11] = r.rname2_len;
  w[12] = (uint32_t)r.rname2_off;
  w[13] = (uint32_t)(r.rname2_off >> 32);
  w[14] = r.v0, w[15] = r.v1, w[16] = r.v2, w[17] = r.v3, w[18] = r.v4;
  w[19] = r.v5, w[20] = r.v6, w[21] = r.v7, w[22] = r.v8, w[23] = r.v9;
}

// the one RDATA name of most typed forms: into rname, the cursor moves on
template <bool kEmit, typename B>
GPK_HD uint32_t rdata_name(const B& d, uint32_t end, uint32_t off, Cur& c, Rr& r, uint32_t& endq) {
  uint32_t n;
  if (const uint32_t e = decode_name<kEmit>(d, end, off, c, n, endq)) return e;
  r.rname_off = c.pos;
  r.rname_len = n;
  c.pos += n;
  return 0;
}

// NAPTR's three character-strings (:1457-1489): missing, then truncated
template <typename B>
GPK_HD uint32_t naptr_string(const B& d, uint32_t end, uint32_t& off, uint32_t hdr_off, uint32_t& v_off,
                             uint32_t& v_len, uint32_t missing, uint32_t truncated) {
  if (end < off + 1) return missing;
  const uint32_t l = d[off];
  off++;
  if (end < off + l) return truncated;
  v_off = hdr_off + off;
  v_len = l;
  off += l;
  return 0;
}

// decodeRData(data[:end], off, buffer); r.type, r.data_length (> 0) and r.data_off are set
template <bool kEmit, typename B>
GPK_HD uint32_t rdata(const B& d, uint32_t end, uint32_t off, uint32_t hdr_off, Cur& c, Rr& r) {
  uint32_t endq;
  switch (r.type) {
    case 16:
    case 13: {  // TXT, HINFO: decodeCharacterStrings(rr.Data), :1267-1278
      for (uint32_t i = off; i != end;) {
        const uint32_t i2 = i + 1 + d[i];
        if (i2 > end) return GPK_DNS_ERR_CHARSTRING;
        r.count++;
        i = i2;
      }
      return 0;
    }
    case 2:
    case 5:
    case 12: return rdata_name<kEmit>(d, end, off, c, r, endq);  // NS, CNAME, PTR
    case 6: {                                                   // SOA, :1390-1414
      if (const uint32_t e = rdata_name<kEmit>(d, end, off, c, r, endq)) return e;
      uint32_t n;
      if (const uint32_t e = decode_name<kEmit>(d, end, endq, c, n, endq)) return e;
      if (end < endq + 20) return GPK_DNS_ERR_SOA_SMALL;
      r.rname2_off = c.pos;
      r.rname2_len = n;
      c.pos += n;
      r.v0 = be32(d + endq), r.v1 = be32(d + endq + 4), r.v2 = be32(d + endq + 8);
      r.v3 = be32(d + endq + 12), r.v4 = be32(d + endq + 16);
      return 0;
    }
    case 15:  // MX, :1415-1427
      if (end < off + 2) return GPK_DNS_ERR_MX_SMALL;
      r.v0 = be16(d + off);
      return rdata_name<kEmit>(d, end, off + 2, c, r, endq);
    case 256:  // URI, :1428-1434
      if (r.data_length < 4) return GPK_DNS_ERR_URI_SMALL;
      r.v0 = be16(d + off), r.v1 = be16(d + off + 2);
      return 0;
    case 33:  // SRV, :1435-1449
      if (end < off + 6) return GPK_DNS_ERR_SRV_SMALL;
      r.v0 = be16(d + off), r.v1 = be16(d + off + 2), r.v2 = be16(d + off + 4);
      return rdata_name<kEmit>(d, end, off + 6, c, r, endq);
    case 35: {  // NAPTR, :1450-1498
      if (end < off + 4) return GPK_DNS_ERR_NAPTR_SMALL;
      r.v0 = be16(d + off), r.v1 = be16(d + off + 2);
      off += 4;
      if (const uint32_t e = naptr_string(d, end, off, hdr_off, r.v2, r.v3, GPK_DNS_ERR_NAPTR_FLAGS_MISSING,
                                          GPK_DNS_ERR_NAPTR_FLAGS_TRUNC))
        return e;
      if (const uint32_t e = naptr_string(d, end, off, hdr_off, r.v4, r.v5, GPK_DNS_ERR_NAPTR_SERVICE_MISSING,
                                          GPK_DNS_ERR_NAPTR_SERVICE_TRUNC))
        return e;
      if (const uint32_t e = naptr_string(d, end, off, hdr_off, r.v6, r.v7, GPK_DNS_ERR_NAPTR_REGEXP_MISSING,
                                          GPK_DNS_ERR_NAPTR_REGEXP_TRUNC))
        return e;
      return rdata_name<kEmit>(d, end, off, c, r, endq);
    }
    case 41: {  // OPT: decodeOPTs, :1280-1307 (offset == end needs DataLength 0: not reached)
      if (off + 4 > end) {
        c.a0 = end - off;
        return GPK_DNS_ERR_OPT_LENGTH;
      }
      for (uint32_t i = off; i < end;) {
        if (end < i + 4) {
          c.a0 = end;
          c.a1 = i + 4;
          return GPK_DNS_ERR_OPT_MALFORMED;
        }
        const uint32_t l = be16(d + i + 2);
        if (i + 4 + l > end) {
          c.a0 = l;
          return GPK_DNS_ERR_OPT_IMPLIES;
        }
        r.count++;
        i += l + 4;
      }
      return 0;
    }
    case 46: {  // RRSIG, :1726-1748; the signer's strip leaves the plain join (gpk_dns.h, RRSIG)
      if (end < off + 18) return GPK_DNS_ERR_RRSIG_SMALL;
      r.v0 = be16(d + off), r.v1 = d[off + 2], r.v2 = d[off + 3];
      r.v3 = be32(d + off + 4), r.v4 = be32(d + off + 8), r.v5 = be32(d + off + 12);
      r.v6 = be16(d + off + 16);
      if (const uint32_t e = rdata_name<kEmit>(d, end, off + 18, c, r, endq)) return e;
      r.v7 = hdr_off + endq;
      r.v8 = end - endq;
      return 0;
    }
    case 48:  // DNSKEY, :1815-1824
      if (end < off + 4) return GPK_DNS_ERR_DNSKEY_SMALL;
      r.v0 = be16(d + off), r.v1 = d[off + 2], r.v2 = d[off + 3];
      return 0;
    case 64:
    case 65: {  // SVCB, HTTPS: decodeSVCB, :1309-1348 (offset == end: not reached)
      if (off + 3 > end) {
        c.a0 = end - off;
        return GPK_DNS_ERR_SVCB_LENGTH;
      }
      r.v0 = be16(d + off);
      if (const uint32_t e = rdata_name<kEmit>(d, end, off + 2, c, r, endq)) return e;
      r.v1 = hdr_off + endq;
      for (uint32_t o = endq; o < end;) {
        if (o + 4 > end) return GPK_DNS_ERR_SVCB_TRUNC;
        const uint32_t l = be16(d + o + 2);
        if (o + 4 + l > end) return GPK_DNS_ERR_SVCB_TRUNC;
        r.count++;
        o += 4 + l;
      }
      return 0;
    }
    default: return 0;  // A, AAAA (IP is Data) and every other type
  }
}

GPK_HD void fail(Msg& m, uint32_t code, uint32_t a0, uint32_t a1) {
  msg_init(m, m.hdr_off);
  m.err = code;
  m.a0 = a0;
  m.a1 = a1;
  m.status = code == GPK_DNS_ERR_SHORT ? GPK_DNS_ST_TRUNCATED : 0u;
}

// DNS.DecodeFromBytes(d[:len]). kEmit: entry k of the message goes to rrs[k],
// its names to names + name0 on (the caller has checked that both fit).
template <bool kEmit, typename B>
GPK_HD void walk(const B& d, uint32_t len, Msg& m, gpk_dns_rr* rrs, uint8_t* names, uint64_t name0) {
  if (len < 12) return fail(m, GPK_DNS_ERR_SHORT, 0, 0);
  m.len = len;
  m.id = be16(d);
  m.flags2 = d[2];
  m.flags3 = d[3];
  m.rcode = d[3] & 0xFu;
  m.qd = be16(d + 4), m.an = be16(d + 6), m.ns = be16(d + 8), m.ar = be16(d + 10);
  Cur c{names, name0, 0, 0};
  uint32_t offset = 12, k = 0;
  for (uint32_t section = 0; section < 4; section++) {
    const uint32_t count = section == 0 ? m.qd : section == 1 ? m.an : section == 2 ? m.ns : m.ar;
    for (uint32_t i = 0; i < count; i++, k++) {
      Rr r;
      rr_init(r, section);
      uint32_t n, endq;
      if (const uint32_t e = decode_name<kEmit>(d, len, offset, c, n, endq)) return fail(m, e, c.a0, c.a1);
      r.name_off = c.pos;
      r.name_len = n;
      c.pos += n;
      if (section == 0) {  // DNSQuestion.decode, :933-952
        if (len < endq + 4) return fail(m, GPK_DNS_ERR_QUESTION_SMALL, 0, 0);
        r.type = be16(d + endq);
        r.cls = be16(d + endq + 2);
        offset = endq + 4;
      } else {  // DNSResourceRecord.decode, :1056-1087
        if (len < endq + 10) return fail(m, GPK_DNS_ERR_RECORD_SMALL, 0, 0);
        r.type = be16(d + endq);
        r.cls = be16(d + endq + 2);
        r.ttl = be32(d + endq + 4);
        r.data_length = be16(d + endq + 8);
        const uint32_t end = endq + 10 + r.data_length;
        if (end > len) return fail(m, GPK_DNS_ERR_RECORD_LENGTH, 0, 0);
        r.data_off = m.hdr_off + endq + 10;
        if (r.data_length)
          if (const uint32_t e = rdata<kEmit>(d, end, endq + 10, m.hdr_off, c, r)) return fail(m, e, c.a0, c.a1);
        offset = end;
        if (section == 3 && r.type == 41) m.rcode = (m.rcode | (r.ttl >> 20 & 0xF0u)) & 0xFFu;  // :406-408
      }
      if (kEmit) rr_store(rrs + k, r);
    }
  }
  m.nrr = k;
  m.name_bytes = c.pos - name0;
}

// One packet of gpk_dns_batch: the class (GPK_DNS_CLASS_*), GPK_DNS_NONE or
// GPK_DNS_UNKNOWN; m is written for a class.
GPK_HD int dns(const DevTables* T, const uint8_t* p, uint32_t caplen, const gpk_record& rec, const gpk_layout& L,
               Msg& m) {
  static_assert(GPK_DNS_NONE == GPK_TUN_NONE && GPK_DNS_UNKNOWN == GPK_TUN_UNKNOWN, "tun::candidate's verdicts");
  tun::Pay pay;
  if (const int no = tun::candidate(T, p, caplen, rec, L, pay)) return no;
  if (pay.next != GPK_LT_DNS) return GPK_DNS_NONE;
  msg_init(m, pay.off);
  walk<false>(p + pay.off, pay.len, m, nullptr, nullptr, 0);
  return m.err ? GPK_DNS_CLASS_FAILED : GPK_DNS_CLASS_OK;
}

}  // namespace dns
}  // namespace gpk
