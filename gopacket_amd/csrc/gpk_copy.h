// gpk_copy.h — the byte mover of the reassembly kernels (gpk_defrag.hip,
// gpk_defrag6.hip): dst[0..n) = src[0..n) by one wave, with destination-aligned
// 16-byte stores, the source realigned in registers from two aligned loads, and
// a byte head and tail.
#ifndef GPK_COPY_H
#define GPK_COPY_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gpk {

// Every 16-byte load is aligned and holds at least one byte of the source, so
// it stays inside the pages the source is in.
template <int Q>
__device__ __forceinline__ void copy_vectors(uint4* d, const uint4* sa, uint32_t nvec, uint32_t r, uint32_t lane) {
  for (uint32_t v = lane; v < nvec; v += 64) {
    const uint4 A = sa[v], B = sa[v + 1];
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    uint4 out;
    out.x = (uint32_t)((((uint64_t)w[Q + 1] << 32) | w[Q]) >> r);
    out.y = (uint32_t)((((uint64_t)w[Q + 2] << 32) | w[Q + 1]) >> r);
    out.z = (uint32_t)((((uint64_t)w[Q + 3] << 32) | w[Q + 2]) >> r);
    out.w = (uint32_t)((((uint64_t)w[Q + 4] << 32) | w[Q + 3]) >> r);
    d[v] = out;
  }
}

__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
  uint32_t head = (uint32_t)(-(uintptr_t)dst & 15);
  if (head > n) head = n;
  const uint32_t body = n - head, nvec = body >> 4, tail = body & 15;
  uint8_t* d16 = dst + head;
  const uint8_t* s16 = src + head;
  if (lane < head) dst[lane] = src[lane];
  if (lane >= 16 && lane < 16 + tail) d16[nvec * 16 + lane - 16] = s16[nvec * 16 + lane - 16];
  if (!nvec) return;
  const uint32_t sh = (uint32_t)((uintptr_t)s16 & 15);
  const uint4* sa = (const uint4*)(s16 - sh);
  uint4* d = (uint4*)d16;
  if (sh == 0) {
    for (uint32_t v = lane; v < nvec; v += 64) d[v] = sa[v];
    return;
  }
  const uint32_t r = (sh & 3) * 8;
  switch (sh >> 2) {  // wave-uniform: one source phase per segment
    case 0: copy_vectors<0>(d, sa, nvec, r, lane); break;
    case 1: copy_vectors<1>(d, sa, nvec, r, lane); break;
    case 2: copy_vectors<2>(d, sa, nvec, r, lane); break;
    default: copy_vectors<3>(d, sa, nvec, r, lane); break;
  }
}

}  // namespace gpk
#endif  // GPK_COPY_H
