// gpk_copy.h — the byte mover of every pipeline that moves packet bytes
// (gpk_defrag.hip, gpk_defrag6.hip, gpk_tcpasm.hip, gpk_capwrite.hip,
// gpk_serialize.hip): dst[0..n) = src[0..n) by a group of G lanes (a wave, or
// 16 lanes for small packets), with destination-aligned 16-byte stores, the
// source realigned in registers from two aligned loads, and a byte head and
// tail. With SUM the group also adds the bytes it stores at even and at odd
// addresses into ev / od, per lane (the caller reduces them).
//
// Page safety: the body's loads are aligned 16-byte loads of sa[v] and
// sa[v + 1] for v < nvec, where sa is the source of the body rounded down to 16
// bytes. sa[v + 1] is read only when the source is not aligned (sh != 0), and
// then it holds the last sh bytes of the body's vector v; sa[v] always holds its
// first bytes. So every load holds at least one byte of the source and, being
// aligned, stays inside the pages the source is in. Head and tail are byte
// loads of the source itself.
//
// Lanes: the head (at most 15 bytes, up to the destination's alignment) goes
// to lanes 0..; the tail (at most 15 bytes) to lanes 16.. of a wave, so that
// head and tail go out together, and to lanes 0.. of a 16-lane group, which has
// no others. The lanes' stores never overlap.
#ifndef GPK_COPY_H
#define GPK_COPY_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gpk {

template <bool SUM>
__device__ __forceinline__ void add_vec(const uint4& v, uint32_t& ev, uint32_t& od) {
  if (!SUM) return;
  ev = __builtin_amdgcn_udot4(v.x, 0x00010001u, ev, false);
  od = __builtin_amdgcn_udot4(v.x, 0x01000100u, od, false);
  ev = __builtin_amdgcn_udot4(v.y, 0x00010001u, ev, false);
  od = __builtin_amdgcn_udot4(v.y, 0x01000100u, od, false);
  ev = __builtin_amdgcn_udot4(v.z, 0x00010001u, ev, false);
  od = __builtin_amdgcn_udot4(v.z, 0x01000100u, od, false);
  ev = __builtin_amdgcn_udot4(v.w, 0x00010001u, ev, false);
  od = __builtin_amdgcn_udot4(v.w, 0x01000100u, od, false);
}

// a wave, the source phase Q (words) and r (bits) wave-uniform
template <int Q, bool SUM>
__device__ __forceinline__ void copy_vectors(uint4* d, const uint4* sa, uint32_t nvec, uint32_t r, uint32_t lane,
                                             uint32_t& ev, uint32_t& od) {
  for (uint32_t v = lane; v < nvec; v += 64) {
    const uint4 A = sa[v], B = sa[v + 1];
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    uint4 out;
    out.x = (uint32_t)((((uint64_t)w[Q + 1] << 32) | w[Q]) >> r);
    out.y = (uint32_t)((((uint64_t)w[Q + 2] << 32) | w[Q + 1]) >> r);
    out.z = (uint32_t)((((uint64_t)w[Q + 3] << 32) | w[Q + 2]) >> r);
    out.w = (uint32_t)((((uint64_t)w[Q + 4] << 32) | w[Q + 3]) >> r);
    d[v] = out;
    add_vec<SUM>(out, ev, od);
  }
}

__device__ __forceinline__ uint32_t pick4(uint32_t q, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return q == 0 ? a : q == 1 ? b : q == 2 ? c : d;
}

// 16 lanes, the phase a per-lane value: the five words are selected
template <bool SUM>
__device__ __forceinline__ void copy_vectors_sel(uint4* d, const uint4* sa, uint32_t nvec, uint32_t sh, uint32_t lane,
                                                 uint32_t& ev, uint32_t& od) {
  const uint32_t q = sh >> 2, r = (sh & 3) * 8;
  for (uint32_t v = lane; v < nvec; v += 16) {
    const uint4 A = sa[v];
    uint4 B = A;
    if (sh) B = sa[v + 1];  // an aligned source has no byte in the next word
    const uint32_t w0 = pick4(q, A.x, A.y, A.z, A.w), w1 = pick4(q, A.y, A.z, A.w, B.x),
                   w2 = pick4(q, A.z, A.w, B.x, B.y), w3 = pick4(q, A.w, B.x, B.y, B.z),
                   w4 = pick4(q, B.x, B.y, B.z, B.w);
    uint4 out;
    out.x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> r);
    out.y = (uint32_t)((((uint64_t)w2 << 32) | w1) >> r);
    out.z = (uint32_t)((((uint64_t)w3 << 32) | w2) >> r);
    out.w = (uint32_t)((((uint64_t)w4 << 32) | w3) >> r);
    d[v] = out;
    add_vec<SUM>(out, ev, od);
  }
}

template <int G, bool SUM>
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane, uint32_t& ev,
                                           uint32_t& od) {
  static_assert(G == 64 || G == 16, "a wave or a 16-lane group");
  uint32_t head = (uint32_t)(-(uintptr_t)dst & 15);
  if (head > n) head = n;
  const uint32_t body = n - head, nvec = body >> 4, tail = body & 15;
  uint8_t* d16 = dst + head;
  const uint8_t* s16 = src + head;
  constexpr uint32_t kTailLane = G == 64 ? 16 : 0;  // head and tail are at most 15 bytes each
  if (lane < head) {
    const uint32_t b = src[lane];
    dst[lane] = (uint8_t)b;
    if (SUM) { if ((uintptr_t)(dst + lane) & 1) od += b; else ev += b; }
  }
  if (lane >= kTailLane && lane < kTailLane + tail) {
    const uint32_t k = nvec * 16 + lane - kTailLane;
    const uint32_t b = s16[k];
    d16[k] = (uint8_t)b;
    if (SUM) { if (k & 1) od += b; else ev += b; }  // d16 is 16-byte aligned here (or the body is empty and so is the tail)
  }
  if (!nvec) return;
  const uint32_t sh = (uint32_t)((uintptr_t)s16 & 15);
  const uint4* sa = (const uint4*)(s16 - sh);
  uint4* d = (uint4*)d16;
  if (G == 16) {
    copy_vectors_sel<SUM>(d, sa, nvec, sh, lane, ev, od);
    return;
  }
  if (sh == 0) {
    for (uint32_t v = lane; v < nvec; v += 64) {
      const uint4 x = sa[v];
      d[v] = x;
      add_vec<SUM>(x, ev, od);
    }
    return;
  }
  const uint32_t r = (sh & 3) * 8;
  switch (sh >> 2) {  // wave-uniform: one source per wave
    case 0: copy_vectors<0, SUM>(d, sa, nvec, r, lane, ev, od); break;
    case 1: copy_vectors<1, SUM>(d, sa, nvec, r, lane, ev, od); break;
    case 2: copy_vectors<2, SUM>(d, sa, nvec, r, lane, ev, od); break;
    default: copy_vectors<3, SUM>(d, sa, nvec, r, lane, ev, od); break;
  }
}

// no sums: a group of G lanes, and a whole wave
template <int G>
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
  uint32_t ev = 0, od = 0;
  copy_bytes<G, false>(dst, src, n, lane, ev, od);
}

__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
  copy_bytes<64>(dst, src, n, lane);
}

}  // namespace gpk
#endif  // GPK_COPY_H
