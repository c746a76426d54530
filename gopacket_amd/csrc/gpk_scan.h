// gpk_scan.h — what the pipelines' hipcub scans share (library-internal): the
// two input functors, and the size of one temp buffer that serves every scan
// of a handle.
#ifndef GPK_SCAN_H
#define GPK_SCAN_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

// In an unnamed namespace, as they were in each source: the functor is part of
// the name of every hipcub kernel instantiated with it, and those kernels stay
// each source's own, under the names they had.
namespace {

struct NonZero {  // counts: a scan of these numbers the non-zero entries
  __host__ __device__ uint32_t operator()(uint32_t v) const { return v != 0; }
};
struct Widen {  // sizes: 32-bit lengths summed into 64-bit offsets
  __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

}  // namespace

namespace gpk {

// the largest of the temp sizes hipcub asked for (never an empty allocation)
inline size_t max_temp(std::initializer_list<size_t> sizes) { return std::max(std::max(sizes), (size_t)16); }

}  // namespace gpk
#endif  // GPK_SCAN_H
