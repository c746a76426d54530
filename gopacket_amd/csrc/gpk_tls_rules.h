// gpk_tls_rules.h — the per-message rules of gpk_tls_batch, shared by the
// kernels and gpk_tls_batch_host (one __host__ __device__ source, so the CPU
// suite checks the code the device runs). include/gpk_tls.h states the rules
// with the reference's line numbers.
//
//   client_hello   TLSHandshakeRecordClientHello.decodeFromBytes over the body
//                  re-sliced to the end of the packet, with the extension walk
//   record<kStore> one round of decodeTLSRecords: the header checks and the
//                  per-type decode of one record, in two modes of one function:
//                  size only (error, the counts and the server name bytes), and
//                  store (the gpk_tls_rec and gpk_tls_hello entry and the server
//                  name as well). The per-packet walk and the stream walk of
//                  gpk_tls_streams.hip both call it.
//   walk<kStore>   TLS.DecodeFromBytes: decodeTLSRecords as a loop over record
//   Seam           (gpk_seam.h) the bytes of two buffers end to end, for the one record of
//                  a stream that straddles the carried tail and the new bytes
// The functions that read bytes take them as B: a const uint8_t*, or a Seam.
//   tls            one packet: tun::candidate, then walk<false>
// The lane's state is scalars only: no array is indexed at run time.
#pragma once
#include <stdint.h>

#include "../../include/gpk_tls.h"
#include "gpk_seam.h"
#include "gpk_tunnel_rules.h"

namespace gpk {
namespace tls {

using tun::be16;

using gpk::Seam;  // gpk_seam.h

// A gpk_tls being decoded, one dword per field (as dns::Msg)
struct Msg {
  uint32_t err, a0, a1, status, hdr_off, len, nccs, nalert, nhs, napp, nhello;
  uint64_t sni_bytes;
};

GPK_HD void msg_init(Msg& m, uint32_t hdr_off) {
  m.err = m.a0 = m.a1 = m.status = m.len = m.nccs = m.nalert = m.nhs = m.napp = m.nhello = 0;
  m.hdr_off = hdr_off;
  m.sni_bytes = 0;
}

// the packed record (include/gpk_tls.h) as 20 little-endian dwords; rec0, hello0 and sni0 are the emit step's
GPK_HD void msg_store(gpk_tls* dst, const Msg& m) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = m.err | m.status << 8;
  w[1] = m.a0;
  w[2] = m.a1;
  w[3] = m.hdr_off;
  w[4] = m.len;
  w[5] = m.nccs + m.nalert + m.nhs + m.napp;
  w[6] = m.nccs;
  w[7] = m.nalert;
  w[8] = m.nhs;
  w[9] = m.napp;
  w[10] = m.nhello;
  w[11] = 0;
  w[12] = (uint32_t)m.sni_bytes;
  w[13] = (uint32_t)(m.sni_bytes >> 32);
  w[14] = w[15] = w[16] = w[17] = w[18] = w[19] = 0;
}

GPK_HD bool truncates(uint32_t code) {
  return code != GPK_TLS_ERR_RECORD_TYPE && code != GPK_TLS_ERR_HANDSHAKE_TYPE && code != GPK_ERR_PANIC_SLICE_B;
}

GPK_HD void fail(Msg& m, uint32_t code, uint32_t a0, uint32_t a1) {
  msg_init(m, m.hdr_off);
  m.err = code;
  m.a0 = a0;
  m.a1 = a1;
  m.status = truncates(code) ? GPK_TLS_ST_TRUNCATED : 0u;
}

// A gpk_tls_hello being decoded; offsets relative to the packet
struct Hello {
  uint32_t type, sid_len, cm_len, has_sni, length, version, cs_len, ext_len;
  uint32_t random_off, sid_off, cs_off, cm_off, ext_off, sni_off, sni_len;
  uint32_t a0, a1;  // the arguments of a panic text
};

GPK_HD void hello_store(gpk_tls_hello* dst, const Hello& h, uint32_t pkt, uint64_t sni_pos) {
  uint32_t* w = reinterpret_cast<uint32_t*>(dst);
  w[0] = h.type | h.sid_len << 8 | h.cm_len << 16 | h.has_sni << 24;
  w[1] = h.length;
  w[2] = h.version | h.cs_len << 16;
  w[3] = h.ext_len;
  w[4] = pkt;
  w[5] = h.random_off;
  w[6] = h.sid_off;
  w[7] = h.cs_off;
  w[8] = h.cm_off;
  w[9] = h.ext_off;
  w[10] = h.sni_off;
  w[11] = h.sni_len;
  w[12] = (uint32_t)sni_pos;
  w[13] = (uint32_t)(sni_pos >> 32);
  w[14] = w[15] = 0;
}

// decodeFromBytes(data[:cap(data)]) of a ClientHello: d is the record's body at
// packet offset body_off, avail the bytes from there to the end of the packet.
template <typename B>
GPK_HD uint32_t client_hello(const B& d, uint32_t avail, uint32_t body_off, Hello& h) {
  h.has_sni = h.sni_off = h.sni_len = h.a0 = h.a1 = 0;
  if (avail < 39) return GPK_TLS_ERR_HELLO_SHORT;
  h.type = d[0];
  h.length = (uint32_t)d[1] << 16 | be16(d + 2);
  h.version = be16(d + 4);
  h.random_off = body_off + 6;
  h.sid_len = d[38];
  uint32_t pos = 39 + h.sid_len;
  if (avail < pos + 2) return GPK_TLS_ERR_HELLO_SESSION;
  h.sid_off = body_off + 39;
  h.cs_len = be16(d + pos);
  pos += 2;
  if (avail < pos + h.cs_len + 1) return GPK_TLS_ERR_HELLO_CIPHERS;
  h.cs_off = body_off + pos;
  pos += h.cs_len;
  h.cm_len = d[pos];
  pos++;
  if (avail < pos + h.cm_len + 2) return GPK_TLS_ERR_HELLO_COMPRESSION;
  h.cm_off = body_off + pos;
  pos += h.cm_len;
  h.ext_len = be16(d + pos);
  pos += 2;
  if (avail < pos + h.ext_len) return GPK_TLS_ERR_HELLO_EXTENSIONS;
  h.ext_off = body_off + pos;
  // the walk over data = data[pos : pos+ExtensionsLength]; e: data's start, rem: len(data)
  for (uint32_t e = pos, rem = h.ext_len; rem >= 4;) {
    const uint32_t type = be16(d + e), length = be16(d + e + 2);
    if (rem < 4 + length) break;
    if (type == 0 && rem > 6) {
      const uint32_t list_len = be16(d + e + 4), entry_type = d[e + 6];
      if (list_len > 0 && entry_type == 0 && rem > 8) {
        const uint32_t host_len = be16(d + e + 7);
        if (rem > ((8 + host_len) & 0xFFFFu)) {  // a uint16 sum
          const uint32_t high = (9 + host_len) & 0xFFFFu;  // and another: data[9 : 9+hostnameLength]
          if (high < 9) {
            h.a0 = 9;
            h.a1 = high;
            return GPK_ERR_PANIC_SLICE_B;
          }
          h.has_sni = 1;
          h.sni_off = body_off + e + 9;
          h.sni_len = host_len;
        }
      }
    }
    e += 4 + length;
    rem -= 4 + length;
  }
  return 0;
}

// isEncryptedHandshakeMessage; body holds length >= 16 bytes when it reads them
template <typename B>
GPK_HD bool encrypted_handshake(const B& body, uint32_t length) {
  if (length < 16) return false;
  const uint32_t be24 = (uint32_t)body[1] << 16 | be16(body + 2);
  if (length - be24 != 4u) return true;  // uint32 arithmetic
  const uint32_t t = body[0];
  return !(t <= 3 || (t >= 11 && t <= 16) || t == 20);
}

// One round of decodeTLSRecords (tls.go:130-194): d is at the record's header,
// left the bytes from there to the end of the data, avail those to the end of
// the buffer (>= left), body_off the offset reported for the body. Returns 0 and
// the record's body length in `length`, or the error with its arguments in a0,
// a1. m counts the record; kStore: it goes to *rec, its hello to
// hellos[m.nhello] and its server name to snis + sni0 + m.sni_bytes (the caller
// has checked that they fit); pkt is what the hello entry names.
template <bool kStore, typename B>
GPK_HD uint32_t record(const B& d, uint32_t left, uint32_t avail, uint32_t body_off, Msg& m, uint32_t pkt,
                       gpk_tls_rec* rec, gpk_tls_hello* hellos, uint8_t* snis, uint64_t sni0, uint32_t& length,
                       uint32_t& a0, uint32_t& a1) {
  a0 = a1 = 0;
  if (left < 5) return GPK_TLS_ERR_RECORD_SHORT;
  const uint32_t ct = d[0], version = be16(d + 1);
  length = be16(d + 3);
  if (ct < 20 || ct > 23) return GPK_TLS_ERR_RECORD_TYPE;
  if (left < 5 + length) return GPK_TLS_ERR_LENGTH_MISMATCH;
  const B body = d + 5;
  uint32_t hs = GPK_TLS_HS_NONE, v0 = 0, v1 = 0, hello = GPK_TLS_NO_HELLO;
  if (ct == 20) {
    if (length != 1) return GPK_TLS_ERR_CCS_LENGTH;
    v0 = body[0] == 1 ? 1u : 255u;
    m.nccs++;
  } else if (ct == 21) {
    if (length < 2) return GPK_TLS_ERR_ALERT_SHORT;
    v0 = length == 2 ? body[0] : 255u;
    v1 = length == 2 ? body[1] : 255u;
    m.nalert++;
  } else if (ct == 22) {
    if (encrypted_handshake(body, length)) {
      hs = GPK_TLS_HS_ENCRYPTED;
    } else {
      if (length < 1) return GPK_TLS_ERR_HANDSHAKE_SHORT;
      const uint32_t t = body[0];
      if (t == 1) {
        Hello h;
        if (const uint32_t e = client_hello(body, avail - 5, body_off, h)) {
          a0 = h.a0, a1 = h.a1;
          return e;
        }
        hs = GPK_TLS_HS_CLIENT_HELLO;
        hello = m.nhello;
        if (kStore) {
          const uint64_t at = sni0 + m.sni_bytes;
          hello_store(hellos + m.nhello, h, pkt, at);
          const B src = body + (h.sni_off - body_off);
          for (uint32_t i = 0; i < h.sni_len; i++) snis[at + i] = src[i];
        }
        m.nhello++;
        m.sni_bytes += h.sni_len;
      } else if (t == 16) {
        hs = GPK_TLS_HS_CLIENT_KEY;
      } else {
        return GPK_TLS_ERR_HANDSHAKE_TYPE;
      }
    }
    m.nhs++;
  } else {
    m.napp++;
  }
  if (kStore) {
    uint32_t* w = reinterpret_cast<uint32_t*>(rec);
    w[0] = ct | hs << 8 | v0 << 16 | v1 << 24;
    w[1] = version | length << 16;
    w[2] = body_off;
    w[3] = hello;
  }
  return 0;
}

// TLS.DecodeFromBytes(d[:len]); avail: the bytes from d to the end of the
// packet (>= len). kStore: record k of the message goes to recs[k], hello k to
// hellos[k], the server names to snis + sni0 on (the caller has checked that
// all three fit); pkt is the packet's index.
template <bool kStore>
GPK_HD void walk(const uint8_t* d, uint32_t len, uint32_t avail, Msg& m, uint32_t pkt, gpk_tls_rec* recs,
                 gpk_tls_hello* hellos, uint8_t* snis, uint64_t sni0) {
  m.len = len;
  uint32_t k = 0;
  for (uint32_t off = 0;;) {
    uint32_t length, a0, a1;
    if (const uint32_t e = record<kStore>(d + off, len - off, avail - off, m.hdr_off + off + 5, m, pkt,
                                          kStore ? recs + k : nullptr, hellos, snis, sni0, length, a0, a1))
      return fail(m, e, a0, a1);
    k++;
    off += 5 + length;
    if (off == len) return;
  }
}

// One packet of gpk_tls_batch: the class (GPK_TLS_CLASS_*), GPK_TLS_NONE or
// GPK_TLS_UNKNOWN; m is written for a class.
GPK_HD int tls(const DevTables* T, const uint8_t* p, uint32_t caplen, const gpk_record& rec, const gpk_layout& L,
               Msg& m) {
  static_assert(GPK_TLS_NONE == GPK_TUN_NONE && GPK_TLS_UNKNOWN == GPK_TUN_UNKNOWN, "tun::candidate's verdicts");
  tun::Pay pay;
  if (const int no = tun::candidate(T, p, caplen, rec, L, pay)) return no;
  if (pay.next != GPK_LT_TLS) return GPK_TLS_NONE;
  msg_init(m, pay.off);
  walk<false>(p + pay.off, pay.len, caplen - pay.off, m, 0, nullptr, nullptr, nullptr, 0);
  return m.err ? GPK_TLS_CLASS_FAILED : GPK_TLS_CLASS_OK;
}

}  // namespace tls
}  // namespace gpk
