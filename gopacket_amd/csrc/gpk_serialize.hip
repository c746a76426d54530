// gpk_serialize.hip — gopacket.SerializeLayers for the packets of a device
// batch (include/gpk_serialize.h): the layer list, the per-layer SerializeTo
// and the scope decisions are described there.
//
//   1. size_kernel    one lane per output packet: make_plan() walks the layer
//                     list and gives the status, its arguments, the output
//                     length (0 for a packet in error) and the tail's place:
//                     source offset, length, output offset (12 bytes a packet)
//   2. hipcub scan    exclusive sum of the lengths in uint64: out_offsets[0..m]
//   3. counts_kernel  packets written, bytes needed, packets in error, overflow
//   4. move_kernel    one group of G lanes per output packet, G = 64 (one wave)
//                     or 16 (four packets per wave), as gpk_capwrite.hip's
//                     framing kernel. It reads the tail's place and moves the
//                     tail with destination-aligned 16-byte stores
//                     (gpk_copy.h's copy_bytes<G, SUM>). With ComputeChecksums (a
//                     template parameter, so the plain move carries no sum) the
//                     lanes add up the bytes they store, split by the parity of
//                     the output ADDRESS: even and odd bytes separately, mod
//                     2^32. A 16-byte store starts on an even address, so the
//                     split is the same for every vector, and the big-endian word
//                     sum relative to the L4 header is (even << 8) + odd when that
//                     header starts on an even address and (odd << 8) + even when
//                     not: the byte swap of a segment on an odd offset falls out
//                     of the addresses. The group reduces the two sums with xor
//                     shuffles inside the group and stores them (8 bytes a packet).
//   5. head_kernel    one lane per output packet again: the plan is not stored
//                     but computed a second time (a few dependent loads of header
//                     bytes, cheap when 64 packets share a wave, dear when the 16
//                     or 64 lanes of a mover group all wait for them). The lane reads
//                     the fields record as 32 dwords, builds the headers from it
//                     and the source option bytes, stores them as aligned dwords
//                     (WordSink), adds the header words, the pseudo-header and the
//                     tail's sums, folds, writes the L4 checksum and the IPv4
//                     header checksum, copies the gaps (the few bytes of an outer
//                     stacked header) and zeroes the Ethernet pad.
// No per-lane array is indexed at run time, so there is no scratch.
// The host version (gpk_serialize_batch_host) runs the same plan and the same
// header builders in a loop.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/gpk_serialize.h"
#include "gpk_copy.h"
#include "gpk_devguard.h"
#include "gpk_scan.h"

namespace {

#define GPK_HD __host__ __device__ __forceinline__

// batches whose mean packet is at most this many bytes take the 16-lane move kernel.
// Measured (tools/serialize_bench.py, profiles/serialize.json): 16 lanes
// per packet win up to tails of 1500 bytes, 64 lanes from 2048 bytes on, as in the
// capture writer.
constexpr uint64_t kGroup16MaxMean = 1792;

constexpr int kEth = 0, kD1q = 1, kIp4 = 2, kIp6 = 3, kTcp = 4, kUdp = 5, kKinds = 6, kNone = 7;
constexpr uint32_t kAbsent = GPK_LAYOUT_ABSENT;
GPK_HD constexpr int slot_of(int ki) { return ki < 4 ? ki : ki + 1; }  // layout slot = GPK_DEC_* - 1

struct Pkt {
  const uint8_t* p;
  uint32_t cap;
  GPK_HD uint32_t u8(uint32_t o) const { return p[o]; }
  GPK_HD uint32_t be16(uint32_t o) const { return (uint32_t)p[o] << 8 | p[o + 1]; }
  GPK_HD uint32_t be32(uint32_t o) const { return be16(o) << 16 | be16(o + 2); }
};

GPK_HD uint64_t load40(const uint8_t* m) {
  return (uint64_t)m[0] | (uint64_t)m[1] << 8 | (uint64_t)m[2] << 16 | (uint64_t)m[3] << 24 | (uint64_t)m[4] << 32;
}
GPK_HD uint32_t load24(const uint8_t* m) { return (uint32_t)m[0] | (uint32_t)m[1] << 8 | (uint32_t)m[2] << 16; }
GPK_HD uint32_t ctz64(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }

// FoldChecksum, checksum.go:53-58
GPK_HD uint32_t fold(uint32_t c) {
  while (c > 0xffffu) c = (c >> 16) + (c & 0xffffu);
  return ~c & 0xffffu;
}

// ---- the option lists, from the maps of the fields record ------------------
// IPv4: the bytes the options take (ip4.go:79-93), or ~0u for a map that does
// not describe this packet.
GPK_HD uint32_t ip4_opt_bytes(const Pkt& pkt, uint32_t s, uint64_t map) {
  uint32_t body = 0;
  for (; map; map &= map - 1) {
    const uint32_t b = s + 20 + ctz64(map);
    if (b >= pkt.cap) return ~0u;
    const uint32_t t = pkt.u8(b);
    uint32_t ln = 1;
    if (t > 1) {
      if (b + 1 >= pkt.cap) return ~0u;
      ln = pkt.u8(b + 1);
      if (ln < 2 || b + ln > pkt.cap) return ~0u;
    }
    body += ln;
  }
  return body > 40 ? ~0u : body;
}

struct TcpLens {
  uint32_t optlen, padsrc, padlen;
  bool ok;
};
// TCP: the serialized option bytes (kind 30 keeps two, tcp.go:196-203) and the
// Padding (tcp.go:204-209, 341-344)
GPK_HD TcpLens tcp_lens(const Pkt& pkt, uint32_t s, uint64_t map, bool fix) {
  TcpLens r{0, 0, 0, false};
  uint32_t last_t = 1, last_b = 0;
  for (; map; map &= map - 1) {
    const uint32_t b = s + 20 + ctz64(map);
    if (b >= pkt.cap) return r;
    const uint32_t t = pkt.u8(b);
    uint32_t ln = 1;
    if (t > 1) {
      if (b + 1 >= pkt.cap) return r;
      ln = pkt.u8(b + 1);
      if (ln < 2 || b + ln > pkt.cap) return r;
      if (t == 30) ln = 2;
    }
    r.optlen += ln;
    last_t = t;
    last_b = b;
  }
  if (last_t == 0) {  // the source's bytes after End of options
    const uint32_t hend = s + (pkt.u8(s + 12) >> 4) * 4;
    r.padsrc = last_b + 1;
    r.padlen = hend > r.padsrc ? hend - r.padsrc : 0;
  }
  if (fix && (r.optlen & 3)) r.padlen = 4 - (r.optlen & 3), r.padsrc = ~0u;  // zeros
  r.ok = r.optlen + r.padlen <= 40;
  return r;
}

// HopByHop: the bytes IPv6HopByHop.SerializeTo writes (ip6.go:476-506) without
// an inserted option, or ~0u for a map that does not describe this packet
GPK_HD uint32_t hbh_bytes(const Pkt& pkt, uint32_t h, uint32_t map, bool fix) {
  uint32_t n = 2;
  for (; map; map &= map - 1) {
    const uint32_t b = h + 2 + (uint32_t)__builtin_ctz(map);
    if (b >= pkt.cap) return ~0u;
    if (pkt.u8(b) == 0) {
      n += 2;  // Pad1 is written as 00 00, ip6.go:314-325
      continue;
    }
    if (b + 1 >= pkt.cap || b + 2 + pkt.u8(b + 1) > pkt.cap) return ~0u;
    n += 2 + pkt.u8(b + 1);
  }
  if (n - 2 > 2000) return ~0u;
  return fix ? n + n % 8 : n;  // ip6.go:399-407: length % 8 bytes of padding
}

// the source Contents length of slot ki at s, 0 when it leaves [s, lim)
GPK_HD uint32_t src_hdr(const Pkt& pkt, int ki, uint32_t s, uint32_t lim) {
  uint32_t need = ki == kEth ? 14u : ki == kD1q ? 4u : ki == kIp6 ? 40u : ki == kUdp ? 8u : 20u;
  if (s > lim || lim - s < need) return 0;
  if (ki == kIp4) need = (pkt.u8(s) & 15) * 4;
  if (ki == kTcp) need = (pkt.u8(s + 12) >> 4) * 4;
  if (ki == kIp6 && pkt.u8(s + 6) == 0) {
    if (lim - s < 42) return 0;
    if (pkt.u8(s + 4) | pkt.u8(s + 5)) need = 40 + pkt.u8(s + 41) * 8 + 8;  // not a jumbogram: ip6.go:239-263
  }
  if (need < 20 && (ki == kIp4 || ki == kTcp)) return 0;
  return lim - s < need ? 0 : need;
}

// the value of the first jumbo option of the HopByHop header at h, walked as
// IPv6HopByHop.DecodeFromBytes walks it (ip6.go:509-526); 0 when there is none
GPK_HD uint32_t src_jumbo_len(const Pkt& pkt, uint32_t h, uint32_t lim) {
  const uint32_t actual = pkt.u8(h + 1) * 8 + 8;
  for (uint32_t off = 2; off < actual && h + off < lim;) {
    const uint32_t t = pkt.u8(h + off);
    if (t == 0) {
      off++;
      continue;
    }
    if (h + off + 1 >= lim) break;
    const uint32_t ln = pkt.u8(h + off + 1);
    if (t == 0xC2 && ln == 4 && h + off + 6 <= lim) return pkt.be32(h + off + 2);
    off += 2 + ln;
  }
  return 0;
}

GPK_HD uint32_t clamp_end(uint32_t e, uint32_t s, uint64_t len) { return s + len < e ? (uint32_t)(s + len) : e; }

// the end of LayerPayload() of the innermost slot ki, slice [s, e)
GPK_HD uint32_t tail_end(const Pkt& pkt, int ki, uint32_t s, uint32_t e) {
  if (ki == kEth) {  // ethernet.go:49-61
    const uint32_t t = pkt.be16(s + 12);
    return t < 0x0600 ? clamp_end(e, s, 14ull + t) : e;
  }
  if (ki == kIp4) {  // ip4.go:184-214
    uint32_t ln = pkt.be16(s + 2);
    if (ln == 0) ln = (e - s) & 0xffffu;
    return clamp_end(e, s, ln);
  }
  if (ki == kIp6) {  // ip6.go:239-275
    const uint32_t ln = pkt.be16(s + 4);
    if (pkt.u8(s + 6) == 0) {
      if (ln == 0) return clamp_end(e, s, 40ull + src_jumbo_len(pkt, s + 40, e));
      return clamp_end(e, s, 40ull + pkt.u8(s + 41) * 8 + 8 + ln);
    }
    return clamp_end(e, s, 40ull + ln);
  }
  if (ki == kUdp) {  // udp.go:44-55
    const uint32_t ln = pkt.be16(s + 4);
    return ln >= 8 ? clamp_end(e, s, ln) : e;
  }
  return e;  // Dot1Q, TCP
}

struct Plan {
  int32_t status;
  uint32_t a0, a1;
  uint32_t out_len, body_end, pad;
  uint32_t tail_src, tail_len, tail_pos;
  uint32_t kept;      // bit ki: the layer is serialized
  int net;            // the pseudo-header: kIp4, kIp6 or kNone
  uint32_t eth_word;  // bytes 12-13 of the Ethernet header
  uint32_t spos[kKinds], glen[kKinds], opos[kKinds], osz[kKinds];
};

// len(b.Bytes()) when layer ki's SerializeTo is called
GPK_HD uint32_t after_of(const Plan& p, uint32_t opos, uint32_t osz) {
  return p.body_end - (opos + osz) + ((p.kept >> kEth & 1) && p.opos[kEth] > opos ? p.pad : 0u);
}

// IPv6.SerializeTo's errors in its order (ip6.go:139-194, 476-495, 105-134).
// plen0: len(b.Bytes()) at the call; hbh: the HopByHop's bytes (osz - 40).
GPK_HD int32_t ip6_check(const Pkt& pkt, uint32_t s, const gpk_fields& f, bool fix, uint32_t plen0, uint32_t hbh,
                         uint32_t* a0) {
  const bool has_hbh = pkt.u8(s + 6) == 0;
  const bool jumbo = plen0 > 65535;
  const bool longhbh = has_hbh && pkt.u8(s + 41) > 2;
  uint32_t jat = 0, jlen = 0, jpos = 0;  // the first jumbo option: its source offset, OptionLength, serialized offset
  bool found = false;
  if (has_hbh && !longhbh && jumbo) {
    uint32_t n = 2;
    for (uint32_t map = load24(f.hbh_opt_map); map && !found; map &= map - 1) {
      const uint32_t b = s + 42 + (uint32_t)__builtin_ctz(map);
      const uint32_t t = pkt.u8(b);
      if (t == 0) {
        n += 2;
        continue;
      }
      if (t == 0xC2) found = true, jat = b, jlen = pkt.u8(b + 1), jpos = n;
      n += 2 + pkt.u8(b + 1);
    }
  }
  if (jumbo && !fix) {
    if (!has_hbh) {
      *a0 = plen0;
      return GPK_SER_ERR_IP6_FIT_LEN;
    }
    if (longhbh) return GPK_SER_EHBHLONG;
    if (!found) return GPK_SER_ERR_IP6_JUMBO_MISSING;
    if (jlen != 4) return GPK_SER_ERR_IP6_JUMBO_TLV_LEN;
    if (pkt.be32(jat + 2) <= 65535) return GPK_SER_ERR_IP6_JUMBO_SMALL;
  }
  if (jumbo && fix && !has_hbh) return GPK_SER_EJUMBOADD;
  if (has_hbh) {
    if (longhbh) return GPK_SER_EHBHLONG;
    if (jumbo && fix) {
      // SetJumboLength (ip6.go:539-548): shorter data panics in the reference; an
      // option off its 4n+2 alignment would get a padding option inserted (:374-390)
      if (!found || jlen < 4 || (jpos & 3) != 2) return GPK_SER_EJUMBOADD;
    }
    if (hbh % 8) return GPK_SER_ERR_HBH_MULT8;
    if (jumbo && fix && jlen != 4) {
      *a0 = jlen;
      return GPK_SER_ERR_IP6_JUMBO_TLV_SHORT;
    }
  }
  if (!jumbo && (uint64_t)plen0 + hbh > 65535) return GPK_SER_ERR_IP6_FIT;
  return GPK_SER_OK;
}

GPK_HD Plan make_plan(const Pkt& pkt, const gpk_layout& L, const gpk_fields& f, bool fix, bool csum) {
  Plan p;
  p.status = GPK_SER_OK;
  p.a0 = p.a1 = 0;
  p.out_len = p.body_end = p.pad = p.tail_src = p.tail_len = p.tail_pos = p.kept = p.eth_word = 0;
  p.net = kNone;
  const uint32_t present = f.present;
  uint32_t st[kKinds], en[kKinds];
#pragma unroll
  for (int ki = 0; ki < kKinds; ki++) {
    st[ki] = L.start[slot_of(ki)];
    en[ki] = L.end[slot_of(ki)];
    p.spos[ki] = p.glen[ki] = p.opos[ki] = p.osz[ki] = 0;
  }
#pragma unroll
  for (int ki = 0; ki < kKinds; ki++)
    if ((present >> slot_of(ki) & 1) && st[ki] == kAbsent) p.status = GPK_SER_ENOLAYER;
  if (p.status) return p;

  uint32_t prev = 0, pos = 0, inner_s = 0, inner_lim = 0;
  int inner = kNone;
  int64_t lastkey = -1;
  for (int r = 0; r < kKinds; r++) {
    // the next slice in ascending (start, kind)
    int sel = kNone;
    int64_t best = INT64_MAX;
    uint32_t e = 0;
#pragma unroll
    for (int ki = 0; ki < kKinds; ki++) {
      const int64_t key = (int64_t)st[ki] << 3 | ki;
      if (st[ki] != kAbsent && key > lastkey && key < best) best = key, sel = ki, e = en[ki];
    }
    if (sel == kNone) break;
    lastkey = best;
    const uint32_t s = (uint32_t)(best >> 3);
    const uint32_t lim = e < pkt.cap ? e : pkt.cap;
    const uint32_t hdr = s >= prev ? src_hdr(pkt, sel, s, lim) : 0;
    if (hdr == 0 || inner == kTcp || inner == kUdp) {
      p.status = GPK_SER_ELAYOUT;
      return p;
    }
    const uint32_t glen = s - prev;
    pos += glen;
    uint32_t size = 0;
    if (present >> slot_of(sel) & 1) {
      if (sel == kEth) size = 14;
      if (sel == kD1q) size = 4;
      if (sel == kUdp) size = 8;
      if (sel == kIp4) {
        const uint32_t body = ip4_opt_bytes(pkt, s, load40(f.ip4_opt_map));
        size = body == ~0u ? 0 : 20 + ((body + 3) & ~3u);  // getIPv4OptionSize; Padding is never written
      }
      if (sel == kTcp) {
        const TcpLens t = tcp_lens(pkt, s, load40(f.tcp_opt_map), fix);
        size = t.ok ? 20 + t.optlen + t.padlen : 0;
      }
      if (sel == kIp6) {
        size = 40;
        if (pkt.u8(s + 6) == 0 && pkt.u8(s + 41) <= 2) {
          const uint32_t hb = hbh_bytes(pkt, s + 40, load24(f.hbh_opt_map), fix);
          size = hb == ~0u ? 0 : 40 + hb;
        }
      }
      if (size == 0) {
        p.status = GPK_SER_ELAYOUT;
        return p;
      }
      p.kept |= 1u << sel;
      if (sel == kIp4 || sel == kIp6) p.net = sel;
    }
#pragma unroll
    for (int ki = 0; ki < kKinds; ki++)
      if (ki == sel) p.spos[ki] = s, p.glen[ki] = glen, p.opos[ki] = pos, p.osz[ki] = size;
    pos += size;
    prev = s + hdr;
    inner = sel;
    inner_s = s;
    inner_lim = lim;
  }
  const uint32_t te = inner == kNone ? pkt.cap : tail_end(pkt, inner, inner_s, inner_lim);
  p.tail_src = prev;
  p.tail_len = te > prev ? te - prev : 0;
  p.tail_pos = pos;
  if ((uint64_t)pos + p.tail_len + 60 > 0xffffffffull) {
    p.status = GPK_SER_ELAYOUT;
    return p;
  }
  p.body_end = pos + p.tail_len;
  if (p.kept >> kEth & 1) {
    const uint32_t len = p.body_end - p.opos[kEth];
    p.pad = len < 60 ? 60 - len : 0;  // ethernet.go:95-103
  }
  p.out_len = p.body_end + p.pad;

  // the first error, innermost layer first: the transport layer is the innermost
  if (csum && (p.kept & (1u << kTcp | 1u << kUdp)) && p.net == kNone) {
    p.status = GPK_SER_ERR_L4_NO_NETWORK;
  } else {
    int32_t s6 = GPK_SER_OK, se = GPK_SER_OK;
    uint32_t a6 = 0, ae0 = 0, ae1 = 0;
    if (p.kept >> kIp6 & 1)
      s6 = ip6_check(pkt, p.spos[kIp6], f, fix, after_of(p, p.opos[kIp6], p.osz[kIp6]), p.osz[kIp6] - 40, &a6);
    if (p.kept >> kEth & 1) {  // ethernet.go:82-94
      uint32_t et = f.eth_type, ln = f.eth_length;
      if (ln != 0 || et == 0) {
        if (fix) ln = after_of(p, p.opos[kEth], 14) & 0xffffu;
        if (et != 0)
          se = GPK_SER_ERR_ETH_TYPE_LENGTH, ae0 = et, ae1 = ln;
        else if (ln > 0x0600)
          se = GPK_SER_ERR_ETH_LENGTH, ae0 = ln;
        et = ln;
      }
      p.eth_word = et;
    }
    const bool six_first = s6 && (!se || p.opos[kIp6] > p.opos[kEth]);
    if (six_first)
      p.status = s6, p.a0 = a6;
    else if (se)
      p.status = se, p.a0 = ae0, p.a1 = ae1;
  }
  if (p.status) p.out_len = 0;
  return p;
}

// ---- the header builders: bytes into a sink that also keeps the sum of the
// bytes at even and at odd offsets from the header's start
struct ByteSink {
  uint8_t* d;
  uint32_t pos = 0, se = 0, so = 0;
  GPK_HD explicit ByteSink(uint8_t* out) : d(out) {}
  GPK_HD void put(uint32_t b) {
    b &= 0xffu;
    d[pos] = (uint8_t)b;
    if (pos & 1) so += b; else se += b;
    pos++;
  }
  GPK_HD void be16(uint32_t v) {
    put(v >> 8);
    put(v);
  }
  GPK_HD void be32(uint32_t v) {
    be16(v >> 16);
    be16(v);
  }
  GPK_HD void copy(const uint8_t* s, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) put(s[k]);
  }
  GPK_HD void zeros(uint32_t n) {
    for (uint32_t k = 0; k < n; k++) put(0);
  }
  GPK_HD void finish() {}
  GPK_HD void set16(uint32_t off, uint32_t v) {
    d[off] = (uint8_t)(v >> 8);
    d[off + 1] = (uint8_t)v;
  }
  GPK_HD uint32_t sum() const { return (se << 8) + so; }  // ComputeChecksum of the bytes so far, checksum.go:35-50
};

// The same for the device: the bytes of one header gather in a register and leave
// as whole aligned dwords (a lane of the head kernel has a packet of its own, so
// every store instruction of the wave touches 64 different lines: four times
// fewer stores is four times fewer transactions). The bytes in front of the first
// aligned dword and behind the last leave one by one. A dword store never covers a
// byte outside [d, d + pos).
struct WordSink {
  uint8_t* d;
  uint32_t pos = 0, se = 0, so = 0, acc = 0;
  bool done = false;
  __device__ __forceinline__ explicit WordSink(uint8_t* out) : d(out) {}
  __device__ __forceinline__ void put(uint32_t b) {
    b &= 0xffu;
    const uint32_t k = (uint32_t)((uintptr_t)(d + pos) & 3);
    acc |= b << (k * 8);
    if (pos & 1) so += b; else se += b;
    pos++;
    if (k == 3) {
      if (pos >= 4) {
        *(uint32_t*)(d + pos - 4) = acc;
      } else {  // the header began inside this dword
        for (uint32_t q = 0; q < pos; q++) d[q] = (uint8_t)(acc >> ((4 - pos + q) * 8));
      }
      acc = 0;
    }
  }
  __device__ __forceinline__ void finish() {  // the bytes behind the last whole dword; once
    if (done) return;
    done = true;
    const uint32_t r = (uint32_t)((uintptr_t)(d + pos) & 3);
    const uint32_t have = r < pos ? r : pos;  // bytes of this header in the open dword
    for (uint32_t q = 0; q < have; q++) d[pos - have + q] = (uint8_t)(acc >> ((r - have + q) * 8));
    acc = 0;
  }
  __device__ __forceinline__ void be16(uint32_t v) {
    put(v >> 8);
    put(v);
  }
  __device__ __forceinline__ void be32(uint32_t v) {
    be16(v >> 16);
    be16(v);
  }
  __device__ __forceinline__ void copy(const uint8_t* s, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) put(s[k]);
  }
  __device__ __forceinline__ void zeros(uint32_t n) {
    for (uint32_t k = 0; k < n; k++) put(0);
  }
  __device__ __forceinline__ void set16(uint32_t off, uint32_t v) {  // after the header's last byte
    finish();
    d[off] = (uint8_t)(v >> 8);
    d[off + 1] = (uint8_t)v;
  }
  __device__ __forceinline__ uint32_t sum() const { return (se << 8) + so; }
};

// the IPv4 / TCP options as the maps list them: kinds 0 and 1 one byte, MPTCP
// (kind 30, no OptionData: tcp.go:347-533) two, every other its bytes
template <class S>
GPK_HD void put_options(S& o, const Pkt& pkt, uint32_t s, uint64_t map, bool tcp, bool fix) {
  for (; map; map &= map - 1) {
    const uint32_t b = s + 20 + ctz64(map);
    const uint32_t t = pkt.u8(b);
    if (t <= 1) {
      o.put(t);
    } else if (tcp && t == 30) {
      o.put(30);
      o.put(fix ? 2u : pkt.u8(b + 1));
    } else {
      o.copy(pkt.p + b, pkt.u8(b + 1));
    }
  }
}

// IPv4.SerializeTo, ip4.go:103-169
template <class S>
GPK_HD void put_ip4(S& o, const Pkt& pkt, uint32_t s, const gpk_fields& f, bool fix, bool csum, uint32_t size,
                    uint32_t after) {
  uint32_t ihl = f.ip4_ihl, length = f.ip4_length;
  if (fix) {
    ihl = 5 + (size - 20) / 4;
    length = (size + after) & 0xffffu;  // uint16(len(b.Bytes())): wraps
  }
  o.put((uint32_t)f.ip4_version << 4 | ihl);
  o.put(f.ip4_tos);
  o.be16(length);
  o.be16(f.ip4_id);
  o.be16(f.ip4_flags_frag);
  o.put(f.ip4_ttl);
  o.put(f.ip4_protocol);
  o.be16(0);
#pragma unroll
  for (int k = 0; k < 4; k++) o.put(f.ip4_src[k]);
#pragma unroll
  for (int k = 0; k < 4; k++) o.put(f.ip4_dst[k]);
  put_options(o, pkt, s, load40(f.ip4_opt_map), false, fix);
  o.zeros(size - o.pos);
  o.set16(10, csum ? fold(o.sum()) : (uint32_t)f.ip4_checksum);
}

template <class S>
GPK_HD void put_tlv_padding(S& o, uint32_t n) {  // serializeTLVOptionPadding, ip6.go:348-365
  if (n == 0) return;
  if (n == 1) {
    o.put(0);
    return;
  }
  o.put(1);
  o.put(n - 2);
  o.zeros(n - 2);
}

// IPv6.SerializeTo with its HopByHop, ip6.go:139-218, 476-506
template <class S>
GPK_HD void put_ip6(S& o, const Pkt& pkt, uint32_t s, const gpk_fields& f, bool fix, uint32_t size,
                    uint32_t plen0) {
  const bool has_hbh = size > 40;
  const bool jumbo = plen0 > 65535;
  const uint32_t plen = plen0 + (size - 40);
  uint32_t length = f.ip6_length;
  if (fix) length = jumbo ? 0 : plen & 0xffffu;
  const uint32_t tc = f.ip6_traffic_class, fl = f.ip6_flow_label;
  o.put((uint32_t)f.ip6_version << 4 | tc >> 4);
  o.put(tc << 4 | (fl >> 16 & 0xffu));
  o.be16(fl);
  o.be16(length);
  o.put(has_hbh ? 0u : (uint32_t)f.ip6_next_header);  // ip6.go:173-177
  o.put(f.ip6_hop_limit);
#pragma unroll
  for (int k = 0; k < 16; k++) o.put(f.ip6_src[k]);
#pragma unroll
  for (int k = 0; k < 16; k++) o.put(f.ip6_dst[k]);
  if (!has_hbh) return;
  const uint32_t h = s + 40;
  o.put(pkt.u8(h));
  o.put(fix ? (size - 40) / 8 - 1 : pkt.u8(h + 1));
  bool seen = false;
  for (uint32_t map = load24(f.hbh_opt_map); map; map &= map - 1) {
    const uint32_t b = h + 2 + (uint32_t)__builtin_ctz(map);
    const uint32_t t = pkt.u8(b);
    if (t == 0) {
      o.be16(0);
    } else if (fix && jumbo && t == 0xC2 && !seen) {  // setIPv6PayloadJumboLength, ip6.go:105-134
      seen = true;
      o.put(t);
      o.put(4);
      o.be32(plen);
    } else {
      o.copy(pkt.p + b, 2 + pkt.u8(b + 1));
    }
  }
  if (fix) put_tlv_padding(o, (o.pos - 40) % 8);
}

// TCP.SerializeTo up to the checksum, tcp.go:194-236
template <class S>
GPK_HD void put_tcp(S& o, const Pkt& pkt, uint32_t s, const gpk_fields& f, bool fix) {
  const uint64_t map = load40(f.tcp_opt_map);
  const TcpLens t = tcp_lens(pkt, s, map, fix);
  uint32_t doff = f.tcp_data_offset;
  if (fix) doff = ((t.padlen + t.optlen + 20) / 4) & 0xffu;
  o.be16(f.tcp_src_port);
  o.be16(f.tcp_dst_port);
  o.be32(f.tcp_seq);
  o.be32(f.tcp_ack);
  o.be16((doff << 12 | ((uint32_t)f.tcp_flags & 0x1ffu)) & 0xffffu);
  o.be16(f.tcp_window);
  o.be16(0);
  o.be16(f.tcp_urgent);
  put_options(o, pkt, s, map, true, fix);
  if (t.padsrc == ~0u) o.zeros(t.padlen); else o.copy(pkt.p + t.padsrc, t.padlen);
}

// All headers of a planned packet into dst (the packet's output range). tail_ev,
// tail_od: the sums of the tail's bytes at even and at odd ADDRESSES of dst.
template <class S>
GPK_HD void put_headers(uint8_t* dst, const Pkt& pkt, const gpk_fields& f, const Plan& p, bool fix, bool csum,
                        uint32_t tail_ev, uint32_t tail_od) {
  if (p.kept >> kEth & 1) {
    S o(dst + p.opos[kEth]);
#pragma unroll
    for (int k = 0; k < 6; k++) o.put(f.eth_dst[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) o.put(f.eth_src[k]);
    o.be16(p.eth_word);
    o.finish();
  }
  if (p.kept >> kD1q & 1) {  // dot1q.go:61-76
    S o(dst + p.opos[kD1q]);
    o.be16(f.d1q_tci);
    o.be16(f.d1q_type);
    o.finish();
  }
  if (p.kept >> kIp4 & 1) {
    S o(dst + p.opos[kIp4]);
    put_ip4(o, pkt, p.spos[kIp4], f, fix, csum, p.osz[kIp4], after_of(p, p.opos[kIp4], p.osz[kIp4]));
  }
  if (p.kept >> kIp6 & 1) {
    S o(dst + p.opos[kIp6]);
    put_ip6(o, pkt, p.spos[kIp6], f, fix, p.osz[kIp6], after_of(p, p.opos[kIp6], p.osz[kIp6]));
    o.finish();
  }
  if (p.kept & (1u << kTcp | 1u << kUdp)) {
    const bool tcp = p.kept >> kTcp & 1;
    const uint32_t at = tcp ? p.opos[kTcp] : p.opos[kUdp], size = tcp ? p.osz[kTcp] : 8u;
    const uint32_t after = after_of(p, at, size);
    S o(dst + at);
    uint32_t ck;
    if (tcp) {
      put_tcp(o, pkt, p.spos[kTcp], f, fix);
      ck = f.tcp_checksum;
    } else {  // udp.go:61-105
      const bool jumbo = p.net == kIp6 && after + 8 > 65535;
      uint32_t length = f.udp_length;
      if (fix) length = jumbo ? 0 : (after + 8) & 0xffffu;
      o.be16(f.udp_src_port);
      o.be16(f.udp_dst_port);
      o.be16(length);
      o.be16(0);
      ck = f.udp_checksum;
    }
    if (csum) {
      uint32_t c = 0;  // the pseudo-header, tcpip.go:26-65
      if (p.net == kIp4) {
#pragma unroll
        for (int k = 0; k < 4; k++) c += (uint32_t)f.ip4_src[k] << (k & 1 ? 0 : 8), c += (uint32_t)f.ip4_dst[k] << (k & 1 ? 0 : 8);
      } else {
#pragma unroll
        for (int k = 0; k < 16; k++) c += (uint32_t)f.ip6_src[k] << (k & 1 ? 0 : 8), c += (uint32_t)f.ip6_dst[k] << (k & 1 ? 0 : 8);
      }
      const uint32_t n = size + after;
      c += (tcp ? 6u : 17u) + (n & 0xffffu) + (n >> 16);
      c += o.sum();
      // the tail relative to the transport header's start: same parity of the address = even offset
      const bool even = (((uintptr_t)(dst + at)) & 1) == 0;
      c += even ? (tail_ev << 8) + tail_od : (tail_od << 8) + tail_ev;
      ck = fold(c);
      if (!tcp && ck == 0) ck = 0xffffu;  // RFC 768, udp.go:98-100
    }
    o.set16(tcp ? 16 : 6, ck);
  }
}

// ---- kernels ----------------------------------------------------------------
struct Args {
  uint64_t n, m;
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const gpk_layout* layouts;
  const gpk_fields* fields;
  const uint32_t* order;
  uint32_t fix, csum;
  uint32_t* bsize;  // [m + 1], bsize[m] = 0: the scan's last output is the total
  uint32_t* tails;  // [3m] the tail of output packet j: source offset, length, output offset
  uint32_t* sums;   // [2m] the tail's bytes at even and at odd output addresses, summed
  uint64_t* out_offsets;
  uint32_t* out_caplens;
  int32_t* status;
  uint32_t* err_args;
  uint8_t* out;
  uint64_t cap;
};

__global__ void __launch_bounds__(256) ser_size_kernel(Args a) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > a.m) return;
  if (j == a.m) {
    a.bsize[j] = 0;
    return;
  }
  const uint64_t i = a.order ? a.order[j] : j;
  int32_t st = GPK_SER_EINDEX;
  uint32_t len = 0, a0 = 0, a1 = 0;
  if (i < a.n) {
    const Pkt pkt{a.data + a.offsets[i], a.caplens[i]};
    const Plan p = make_plan(pkt, a.layouts[i], a.fields[i], a.fix, a.csum);
    st = p.status, len = p.out_len, a0 = p.a0, a1 = p.a1;
    a.tails[3 * j] = p.tail_src, a.tails[3 * j + 1] = p.tail_len, a.tails[3 * j + 2] = p.tail_pos;
  }
  a.status[j] = st;
  a.bsize[j] = len;
  a.out_caplens[j] = len;
  if (st && a.err_args) a.err_args[2 * j] = a0, a.err_args[2 * j + 1] = a1;
}

using SizeIt = hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*>;

__global__ void __launch_bounds__(256) ser_counts_kernel(const int32_t* status, const uint64_t* off, uint64_t m,
                                                         uint64_t cap, uint64_t* counts) {
  // a fixed grid strides over the packets; one atomic pair per wave at the end
  uint32_t wrote = 0, errors = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    const int32_t st = status[j];
    wrote += st == GPK_SER_OK && off[j + 1] <= cap;
    errors += st != GPK_SER_OK;
    if (j + 1 == m) {
      counts[1] = off[m];
      counts[3] = off[m] > cap;
    }
  }
  for (int k = 32; k; k >>= 1) {  // every lane of the wave is here
    wrote += (uint32_t)__shfl_xor((int)wrote, k);
    errors += (uint32_t)__shfl_xor((int)errors, k);
  }
  if ((threadIdx.x & 63) == 0) {
    if (wrote) atomicAdd((unsigned long long*)&counts[0], (unsigned long long)wrote);
    if (errors) atomicAdd((unsigned long long*)&counts[2], (unsigned long long)errors);
  }
}

template <int G, bool SUM>
__global__ void __launch_bounds__(256) ser_move_kernel(Args a) {
  constexpr uint32_t kPerBlock = 256 / G;
  const uint32_t lane = threadIdx.x & (G - 1);
  const uint64_t stride = (uint64_t)gridDim.x * kPerBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kPerBlock + threadIdx.x / G; j < a.m; j += stride) {
    const uint64_t at = a.out_offsets[j], end = a.out_offsets[j + 1];
    // a packet in error has no bytes; a packet that does not fit is not written at all
    if (end == at || end > a.cap) continue;
    const uint64_t i = a.order ? a.order[j] : j;  // in range: the size kernel gave this packet a length
    const uint32_t tsrc = a.tails[3 * j], tlen = a.tails[3 * j + 1], tpos = a.tails[3 * j + 2];
    // inside both ranges, whatever the words hold: the size kernel wrote them from this packet's plan
    if ((uint64_t)tpos + tlen > end - at || (uint64_t)tsrc + tlen > a.caplens[i]) continue;
    uint32_t ev = 0, od = 0;
    gpk::copy_bytes<G, SUM>(a.out + at + tpos, a.data + a.offsets[i] + tsrc, tlen, lane, ev, od);
    if (SUM) {
      for (int k = G / 2; k; k >>= 1) {  // inside the group: its lanes are here together
        ev += (uint32_t)__shfl_xor((int)ev, k);
        od += (uint32_t)__shfl_xor((int)od, k);
      }
      if (lane == 0) a.sums[2 * j] = ev, a.sums[2 * j + 1] = od;
    }
  }
}

__global__ void __launch_bounds__(256) ser_head_kernel(Args a) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const uint64_t at = a.out_offsets[j], end = a.out_offsets[j + 1];
  if (end == at || end > a.cap) return;
  const uint64_t i = a.order ? a.order[j] : j;
  const Pkt pkt{a.data + a.offsets[i], a.caplens[i]};
  const gpk_fields f = a.fields[i];  // 32 dword loads into registers, not a byte load per field
  const Plan p = make_plan(pkt, a.layouts[i], f, a.fix, a.csum);
  if (p.status || p.out_len != (uint32_t)(end - at)) return;  // the inputs changed under the call: write nothing
  uint8_t* dst = a.out + at;
  for (uint32_t b = 0; b < p.pad; b++) dst[p.body_end + b] = 0;
#pragma unroll
  for (int ki = 0; ki < kKinds; ki++) {
    const uint8_t* g = pkt.p + p.spos[ki] - p.glen[ki];
    uint8_t* d = dst + p.opos[ki] - p.glen[ki];
    for (uint32_t b = 0; b < p.glen[ki]; b++) d[b] = g[b];
  }
  uint32_t ev = 0, od = 0;
  if (a.csum) ev = a.sums[2 * j], od = a.sums[2 * j + 1];
  put_headers<WordSink>(dst, pkt, f, p, a.fix, a.csum, ev, od);
}

}  // namespace

struct gpk_serializer {
  int device = -1;
  uint64_t cap = 0;
  uint32_t* bsize = nullptr;
  uint32_t* tails = nullptr;  // [3 * cap + 2 * cap]: the tails, then the sums
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
};

extern "C" int gpk_serializer_create(gpk_serializer** out, int device, uint64_t max_packets) {
  if (!out) return GPK_EINVAL;
  if (device >= 0 && (max_packets == 0 || max_packets >= (1ull << 31) - 1)) return GPK_EINVAL;
  gpk_serializer* w = new (std::nothrow) gpk_serializer();
  if (!w) return GPK_ENOMEM;
  if (device >= 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
      delete w;
      return GPK_ENODEV;
    }
    gpk::DeviceScope dscope(device);
    if (dscope.err != hipSuccess) {
      delete w;
      return GPK_EHIP;
    }
    w->device = device;
    w->cap = max_packets;
    size_t tb = 0;
    bool ok = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, SizeIt(nullptr, Widen()), (uint64_t*)nullptr,
                                               (int)(max_packets + 1)) == hipSuccess;
    w->tmp_bytes = std::max(tb, (size_t)16);
    ok = ok && hipMalloc((void**)&w->bsize, (max_packets + 1) * 4) == hipSuccess &&
         hipMalloc((void**)&w->tails, max_packets * 20) == hipSuccess &&
         hipMalloc(&w->tmp, w->tmp_bytes) == hipSuccess;
    if (!ok) {
      if (w->bsize) (void)hipFree(w->bsize);
      if (w->tails) (void)hipFree(w->tails);
      if (w->tmp) (void)hipFree(w->tmp);
      delete w;
      return GPK_ENOMEM;
    }
  }
  *out = w;
  return GPK_OK;
}

extern "C" int gpk_serializer_destroy(gpk_serializer* w) {
  if (!w) return GPK_EINVAL;
  if (w->device >= 0) {
    gpk::DeviceScope dscope(w->device);
    (void)hipDeviceSynchronize();
    if (w->bsize) (void)hipFree(w->bsize);
    if (w->tails) (void)hipFree(w->tails);
    if (w->tmp) (void)hipFree(w->tmp);
  }
  delete w;
  return GPK_OK;
}

namespace {

bool batch_args_ok(const gpk_serializer* w, const gpk_batch* b, const gpk_layout* layouts, const gpk_fields* fields,
                   uint64_t m, const gpk_serialize_opts* opts, uint8_t* out, uint64_t out_cap, uint64_t* out_offsets,
                   uint32_t* out_caplens, int32_t* status, uint64_t* counts) {
  if (!w || !b || !out_offsets || !counts) return false;
  if (m && (!status || !out_caplens || !layouts || !fields)) return false;
  if (m && b->n && (!b->caplens || !b->offsets || !b->data)) return false;
  if (out_cap && !out) return false;
  if (opts && opts->group != 0 && opts->group != 16 && opts->group != 64) return false;
  return true;
}

}  // namespace

extern "C" int gpk_serialize_batch_host(gpk_serializer* w, const gpk_batch* b, const gpk_layout* layouts,
                                        const gpk_fields* fields, const uint32_t* order, uint64_t m,
                                        const gpk_serialize_opts* opts, uint8_t* out, uint64_t out_cap,
                                        uint64_t* out_offsets, uint32_t* out_caplens, int32_t* status,
                                        uint32_t* err_args, uint64_t* counts) {
  if (!batch_args_ok(w, b, layouts, fields, m, opts, out, out_cap, out_offsets, out_caplens, status, counts))
    return GPK_EINVAL;
  const bool fix = opts && opts->fix_lengths, csum = opts && opts->compute_checksums;
  uint64_t at = 0, written = 0, errors = 0;
  out_offsets[0] = 0;
  for (uint64_t j = 0; j < m; j++) {
    const uint64_t i = order ? order[j] : j;
    Plan p;
    p.status = GPK_SER_EINDEX;
    p.out_len = p.a0 = p.a1 = 0;
    Pkt pkt{nullptr, 0};
    if (i < b->n) {
      pkt = Pkt{b->data + b->offsets[i], b->caplens[i]};
      p = make_plan(pkt, layouts[i], fields[i], fix, csum);
    }
    status[j] = p.status;
    out_caplens[j] = p.out_len;
    if (p.status) {
      errors++;
      if (err_args) err_args[2 * j] = p.a0, err_args[2 * j + 1] = p.a1;
    } else if (at + p.out_len <= out_cap) {
      uint8_t* dst = out + at;
      uint32_t ev = 0, od = 0;
      if (p.tail_len) memcpy(dst + p.tail_pos, pkt.p + p.tail_src, p.tail_len);
      if (csum)
        for (uint32_t k = 0; k < p.tail_len; k++) {
          const uint8_t* q = dst + p.tail_pos + k;
          if ((uintptr_t)q & 1) od += *q; else ev += *q;
        }
      if (p.pad) memset(dst + p.body_end, 0, p.pad);
      for (int ki = 0; ki < kKinds; ki++)
        if (p.glen[ki]) memcpy(dst + p.opos[ki] - p.glen[ki], pkt.p + p.spos[ki] - p.glen[ki], p.glen[ki]);
      put_headers<ByteSink>(dst, pkt, fields[i], p, fix, csum, ev, od);
      written++;
    }
    at += p.out_len;
    out_offsets[j + 1] = at;
  }
  counts[0] = written;
  counts[1] = at;
  counts[2] = errors;
  counts[3] = at > out_cap;
  return GPK_OK;
}

extern "C" int gpk_serialize_batch(gpk_serializer* w, const gpk_batch* b, const gpk_layout* layouts,
                                   const gpk_fields* fields, const uint32_t* order, uint64_t m,
                                   const gpk_serialize_opts* opts, uint8_t* out, uint64_t out_cap,
                                   uint64_t* out_offsets, uint32_t* out_caplens, int32_t* status, uint32_t* err_args,
                                   uint64_t* counts, void* stream) {
  if (!batch_args_ok(w, b, layouts, fields, m, opts, out, out_cap, out_offsets, out_caplens, status, counts))
    return GPK_EINVAL;
  if (w->device < 0 || m > w->cap) return GPK_EINVAL;
  const uint32_t group = opts ? opts->group : 0;
  const bool fix = opts && opts->fix_lengths, csum = opts && opts->compute_checksums;
  hipStream_t s = (hipStream_t)stream;
  gpk::DeviceScope dscope(w->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (hipMemsetAsync(counts, 0, 4 * sizeof(uint64_t), s) != hipSuccess) return GPK_EHIP;
  if (m == 0) return hipMemsetAsync(out_offsets, 0, sizeof(uint64_t), s) == hipSuccess ? GPK_OK : GPK_EHIP;
  const dim3 blk(256);
  const Args a{b->n,  m,          b->data,     b->offsets,  b->caplens, layouts,  fields, order, fix,
               csum,  w->bsize,   w->tails,    w->tails + 3 * m, out_offsets, out_caplens, status, err_args,
               out,   out_cap};
  hipLaunchKernelGGL(ser_size_kernel, dim3((unsigned)((m + 1 + 255) / 256)), blk, 0, s, a);
  size_t tb = w->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(w->tmp, tb, SizeIt(w->bsize, Widen()), out_offsets, (int)(m + 1), s) !=
      hipSuccess)
    return GPK_EHIP;
  hipLaunchKernelGGL(ser_counts_kernel, dim3((unsigned)std::min<uint64_t>((m + 255) / 256, 2048)), blk, 0, s, status,
                     out_offsets, m, out_cap, counts);
  // the mean packet size as in gpk_decode_batch: a hint
  const uint64_t mean = b->n && b->data_bytes ? b->data_bytes / b->n : kGroup16MaxMean + 1;
  const bool small = group ? group == 16 : mean <= kGroup16MaxMean;
  const unsigned grid = (unsigned)std::min<uint64_t>(small ? (m + 15) / 16 : (m + 3) / 4, 65536);
  if (small) {
    if (csum)
      hipLaunchKernelGGL((ser_move_kernel<16, true>), dim3(grid), blk, 0, s, a);
    else
      hipLaunchKernelGGL((ser_move_kernel<16, false>), dim3(grid), blk, 0, s, a);
  } else {
    if (csum)
      hipLaunchKernelGGL((ser_move_kernel<64, true>), dim3(grid), blk, 0, s, a);
    else
      hipLaunchKernelGGL((ser_move_kernel<64, false>), dim3(grid), blk, 0, s, a);
  }
  hipLaunchKernelGGL(ser_head_kernel, dim3((unsigned)((m + 255) / 256)), blk, 0, s, a);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

extern "C" int gpk_serialize_format_error(int status, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || !cap) return 0;
  int n = 0;
  switch (status) {
    case GPK_SER_ERR_ETH_TYPE_LENGTH:
      n = snprintf(buf, cap, "ethernet type %u not compatible with length value %u", a0, a1);
      break;
    case GPK_SER_ERR_ETH_LENGTH: n = snprintf(buf, cap, "invalid ethernet length %u", a0); break;
    case GPK_SER_ERR_IP6_FIT_LEN: n = snprintf(buf, cap, "Cannot fit payload length of %u into IPv6 packet", a0); break;
    case GPK_SER_ERR_IP6_JUMBO_MISSING: n = snprintf(buf, cap, "Missing jumbo length hop-by-hop option"); break;
    case GPK_SER_ERR_IP6_JUMBO_TLV_LEN: n = snprintf(buf, cap, "Jumbo length TLV data must have length 4"); break;
    case GPK_SER_ERR_IP6_JUMBO_SMALL: n = snprintf(buf, cap, "Jumbo length cannot be less than 65536"); break;
    case GPK_SER_ERR_IP6_JUMBO_TLV_SHORT: n = snprintf(buf, cap, "Jumbo TLV too short (%u bytes)", a0); break;
    case GPK_SER_ERR_HBH_MULT8: n = snprintf(buf, cap, "IPv6HopByHop actual length must be multiple of 8"); break;
    case GPK_SER_ERR_IP6_FIT: n = snprintf(buf, cap, "Cannot fit payload into IPv6 header"); break;
    case GPK_SER_ERR_L4_NO_NETWORK:
      n = snprintf(buf, cap,
                   "TCP/IP layer 4 checksum cannot be computed without network layer... call "
                   "SetNetworkLayerForChecksum to set which layer to use");
      break;
    default: buf[0] = 0; return 0;
  }
  return n < 0 ? 0 : (size_t)n >= cap ? (int)cap - 1 : n;
}
