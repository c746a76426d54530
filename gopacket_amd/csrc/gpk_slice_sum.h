// gpk_slice_sum.h — ComputeChecksum over a byte slice by a group of lanes
// (library-internal; the GRE sum of gpk_tunnel.hip and the ICMP sums of
// gpk_control.hip).
#ifndef GPK_SLICE_SUM_H
#define GPK_SLICE_SUM_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace gpk {

// Bytes [a, a + len) of data as big-endian 16-bit words from byte a on, summed
// mod 2^32 (ComputeChecksum, checksum.go:35-50: an odd last byte counts as the
// high byte). One dword of a 16-byte chunk at absolute position q; lo/hi bound
// the valid bytes. q is even, so a byte is a word's high byte when its
// position has the parity of a.
__device__ __forceinline__ uint32_t sum_dword(uint32_t w, uint64_t q, uint64_t lo, uint64_t hi, uint32_t odd) {
  uint32_t s = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t b = (w >> (8 * k)) & 0xffu;
    const bool in = q + k >= lo && q + k < hi;
    const bool high = ((k & 1u) ^ odd) == 0;
    s += in ? (high ? b << 8 : b) : 0u;
  }
  return s;
}

// Lane gl of a group of G lanes: its share of the 16-byte chunks that hold bytes [lo, hi).
// The chunks are 16-byte aligned in `data`, so data must be, and the bytes up to the
// next 16-byte boundary past hi must be readable.
template <int G>
__device__ __forceinline__ uint32_t slice_sum(const uint8_t* data, uint64_t lo, uint64_t hi, uint32_t gl) {
  const uint32_t odd = (uint32_t)(lo & 1);
  uint32_t s = 0;
  for (uint64_t q = (lo & ~15ull) + 16ull * gl; q < hi; q += 16ull * G) {
    const uint4 v = *reinterpret_cast<const uint4*>(data + q);
    if (q >= lo && q + 16 <= hi) {  // whole chunk: byte swaps instead of per-byte tests
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t e = w[k] & 0x00ff00ffu, o = (w[k] >> 8) & 0x00ff00ffu;  // bytes 0,2 and 1,3
        const uint32_t hi8 = odd ? o : e, lo8 = odd ? e : o;
        s += ((hi8 & 0xffffu) << 8) + ((hi8 >> 16) << 8) + (lo8 & 0xffffu) + (lo8 >> 16);
      }
    } else {
      s += sum_dword(v.x, q, lo, hi, odd) + sum_dword(v.y, q + 4, lo, hi, odd) +
           sum_dword(v.z, q + 8, lo, hi, odd) + sum_dword(v.w, q + 12, lo, hi, odd);
    }
  }
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d, G);
  return s;
}

}  // namespace gpk
#endif  // GPK_SLICE_SUM_H
