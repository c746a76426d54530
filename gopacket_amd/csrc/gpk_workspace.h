// gpk_workspace.h — the device memory of a pipeline handle and the checks its
// create starts with (library-internal).
//
// A handle's arrays are one device allocation, carved into arrays that each
// start on a 256-byte boundary. The handle names them once, in a carve()
// function made of take(pointer, count) calls. It runs twice: on an empty
// workspace it only adds up the size (and sets null pointers), after alloc()
// it hands out the pointers. One release() frees them all, so no second list
// of the members has to be kept in step.
#ifndef GPK_WORKSPACE_H
#define GPK_WORKSPACE_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/gpk.h"
#include "gpk_devguard.h"

namespace gpk {

struct Workspace {
  uint8_t* base = nullptr;  // null: take() only sizes
  size_t bytes = 0;         // taken so far

  template <typename T>
  void take(T*& p, uint64_t count) {
    p = base ? (T*)(base + bytes) : nullptr;
    bytes += ((size_t)count * sizeof(T) + 255) & ~(size_t)255;
  }
  bool alloc() {  // after the sizing pass: allocate what was taken and start over
    const size_t want = bytes;
    bytes = 0;
    return hipMalloc((void**)&base, want) == hipSuccess;
  }
  void release() {
    if (base) (void)hipFree(base);
    base = nullptr;
    bytes = 0;
  }
};

// What every gpk_*_create checks first (max_packets < limit, as the handle's header documents);
// the caller then opens its DeviceScope (else GPK_EHIP).
inline int check_create(const void* out, int device, uint64_t max_packets, uint64_t limit = 1ull << 28) {
  if (!out || max_packets == 0 || max_packets >= limit) return GPK_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return GPK_ENODEV;
  return GPK_OK;
}

}  // namespace gpk
#endif  // GPK_WORKSPACE_H
