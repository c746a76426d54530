// gpk_postpass.h — a pass over a decoded batch that picks the packets whose
// last layer leads somewhere the parser does not go, decodes what is there and
// writes a compact list ordered by class (library-internal).
// gpk_tunnel.hip and gpk_control.hip are its two users: each supplies a policy
// P and its extern "C" entries.
//
//   1. classify_kernel  one lane per packet: P::decode gives the packet's class;
//                       per 256-packet block the P::kNC class counts and the
//                       number of sums to make, stored row-major
//   2. exclusive scan   of the [kNC + 1][blocks] counts: where each block's
//                       packets of each class start in the compact list (and,
//                       from the last row, how many sums there are: no atomic
//                       counts them), then finish_kernel
//   3. scatter_kernel   one lane per packet again: its rank among the block's
//                       packets of its class (ballots, no atomics: the order is
//                       class, then packet index), then verdict, index and what
//                       P::emit stores at that position
//   4. sum16/64_kernel  16 or 64 lanes per entry that wants a sum: the 16-bit
//                       one's-complement words of Contents‖Payload summed mod
//                       2^32 from 16-byte chunks (gpk_slice_sum.h), plus
//                       P::start, folded once by P::verdict
// The decode runs twice (steps 1 and 3) instead of parking records in a
// workspace: the header bytes are in cache, a record is not.
//
// A policy P supplies
//   Rec, Packed, Out    the lane's working record, the packed entry (it has
//                       hdr_off), the caller's output struct (verdict,
//                       class_start, index, counts and the pass's own arrays)
//   kNC, kNone, kAll, kSumFlag, kSumGroupBytes
//                       classes; the verdict of a lane past the batch; the valid
//                       kinds and the one flag; the default 16/64-lane threshold.
//                       counts[] is m, the kNC class counts, the sums made, zeros
//   decode(a, i, rec)   packet i: its class or a negative verdict  (host + device)
//   wants_sum(rec)      whether the sum step will sum this entry   (host + device)
//   emit(a, i, pos, rec) store the pass's own arrays at pos        (host + device)
//   missing(out)        whether one of those arrays is null
//   entry(out, j)       the packed entry at j
//   entry_wants_sum(packed), entry_len(packed)
//                       wants_sum again, of a stored entry, and the bytes to sum
//   start(sa, packed, pkt, len, gl)
//                       the sum's start value; on the device every lane of a
//                       16-lane group (gl: lane in it) calls it and gets it
//   verdict(packed, sum, start)
//                       write the result into the stored entry
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <new>

#include "gpk_device.h"
#include "gpk_devguard.h"
#include "gpk_slice_sum.h"
#include "gpk_workspace.h"

// gpk_host.cpp: the parser's tables in host memory, and a step enqueued on
// `stream` with their device copy (kept until it completes)
extern "C" __attribute__((visibility("hidden"))) const gpk::DevTables* gpk_parser_tables(const gpk_parser* p);
extern "C" __attribute__((visibility("hidden"))) int gpk_with_device_tables(
    gpk_ctx* c, const gpk_parser* p, void* stream, int (*step)(const gpk::DevTables*, void*), void* arg);

namespace {  // no device symbol is exported

using gpk::slice_sum;

constexpr int kBlk = 256;

template <typename P>
struct PassArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const gpk_record* records;
  const gpk_layout* layouts;
  const gpk::DevTables* tab;
  uint64_t n;
  uint32_t kinds, flags, nblocks;
  uint32_t* block_counts;  // [kNC + 1][nblocks] row-major: the counts (classify), their exclusive sums (scatter)
  typename P::Out out;
};

template <typename P>
struct SumArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const gpk_record* records;
  const gpk_layout* layouts;
  typename P::Out out;
  uint32_t threshold;
};

template <typename P>
__global__ void __launch_bounds__(kBlk) classify_kernel(PassArgs<P> a) {
  constexpr int kNC = P::kNC, kRows = kNC + 1;  // the class counts, then the sums to make
  __shared__ uint32_t cnt[kRows];
  if (threadIdx.x < kRows) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  int cls = P::kNone;
  bool sum = false;
  if (i < a.n) {
    typename P::Rec rec;
    cls = P::decode(a, i, rec);
    sum = cls >= 0 && (a.flags & P::kSumFlag) && P::wants_sum(rec);
  }
#pragma unroll
  for (int c = 0; c < kRows; c++) {
    const uint64_t m = __ballot(c < kNC ? cls == c : sum);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&cnt[c], (uint32_t)__popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < kRows) a.block_counts[(size_t)threadIdx.x * a.nblocks + blockIdx.x] = cnt[threadIdx.x];
}

template <int kNC>
__global__ void finish_kernel(const uint32_t* raw, const uint32_t* scanned, uint32_t nblocks, uint32_t* class_start,
                              uint32_t* counts) {
  // scanned: exclusive sums of the row-major counts raw; a row's start is the total of the rows before it
  if (threadIdx.x == 0) {
    const size_t last = (size_t)(kNC + 1) * nblocks - 1;
    for (int c = 0; c <= kNC; c++) class_start[c] = scanned[(size_t)c * nblocks];
    counts[0] = class_start[kNC];
    for (int c = 0; c < kNC; c++) counts[1 + c] = class_start[c + 1] - class_start[c];
    counts[1 + kNC] = scanned[last] + raw[last] - class_start[kNC];
  }
}

template <typename P>
__global__ void __launch_bounds__(kBlk) scatter_kernel(PassArgs<P> a) {
  constexpr int kNC = P::kNC;
  __shared__ uint32_t wave_cnt[kBlk / 64][kNC];
  const uint64_t i = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int cls = P::kNone;
  typename P::Rec rec;
  if (i < a.n) cls = P::decode(a, i, rec);
  uint32_t rank = 0;
#pragma unroll
  for (int c = 0; c < kNC; c++) {
    const uint64_t m = __ballot(cls == c);
    if (lane == 0) wave_cnt[wave][c] = (uint32_t)__popcll(m);
    if (cls == c) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1));
  }
  __syncthreads();
  if (i >= a.n) return;
  if (cls < 0) {
    a.out.verdict[i] = cls;
    return;
  }
  for (uint32_t w = 0; w < wave; w++) rank += wave_cnt[w][cls];
  const uint32_t pos = a.block_counts[(size_t)cls * a.nblocks + blockIdx.x] + rank;
  a.out.verdict[i] = (int32_t)pos;
  a.out.index[pos] = (uint32_t)i;
  P::emit(a, i, pos, rec);
}

// entries below the threshold: 16 lanes per entry, four entries per wave
template <typename P>
__global__ void __launch_bounds__(kBlk) sum16_kernel(const SumArgs<P> a) {
  constexpr int G = 16;
  const typename P::Out& out = a.out;
  const uint32_t m = out.counts[0];
  const uint32_t gl = threadIdx.x & (G - 1);
  const uint32_t groups = gridDim.x * (kBlk / G);
  for (uint32_t j = blockIdx.x * (kBlk / G) + threadIdx.x / G; j < m; j += groups) {
    typename P::Packed* r = P::entry(out, j);
    if (!P::entry_wants_sum(*r)) continue;
    const uint32_t len = P::entry_len(*r);
    if (len >= a.threshold) continue;
    const uint32_t pkt = out.index[j];
    const uint64_t lo = a.offsets[pkt] + r->hdr_off;
    const uint32_t start = P::start(a, r, pkt, len, gl);
    const uint32_t s = slice_sum<G>(a.data, lo, lo + len, gl);
    if (gl == 0) P::verdict(r, s, start);
  }
}

// entries from the threshold on: a wave looks at 64 entries, one per lane, and
// then sums each of the few long ones with all its lanes
template <typename P>
__global__ void __launch_bounds__(kBlk) sum64_kernel(const SumArgs<P> a) {
  const typename P::Out& out = a.out;
  const uint32_t m = out.counts[0];
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlk / 64);
  for (uint64_t base = ((uint64_t)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6)) * 64; base < m; base += waves * 64) {
    const uint64_t j = base + lane;
    uint32_t len = 0, lo_l = 0, lo_h = 0;
    bool big = false;
    if (j < m) {
      const typename P::Packed* r = P::entry(out, j);
      if (P::entry_wants_sum(*r)) {
        len = P::entry_len(*r);
        big = len >= a.threshold;
        if (big) {
          const uint64_t lo = a.offsets[out.index[j]] + r->hdr_off;
          lo_l = (uint32_t)lo;
          lo_h = (uint32_t)(lo >> 32);
        }
      }
    }
    for (uint64_t todo = __ballot(big); todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const uint64_t lo = (uint64_t)(uint32_t)__shfl((int)lo_h, src) << 32 | (uint32_t)__shfl((int)lo_l, src);
      const uint32_t n = (uint32_t)__shfl((int)len, src);
      typename P::Packed* r = P::entry(out, base + src);
      const uint32_t start = P::start(a, r, out.index[base + src], n, lane & 15);
      const uint32_t s = slice_sum<64>(a.data, lo, lo + n, lane);
      if (lane == 0) P::verdict(r, s, start);
    }
  }
}

// ---- the handle: gpk_tunneler and gpk_controller derive from it

template <typename P>
struct PassHandle {
  using Pass = P;
  int device = 0;
  uint64_t cap = 0;
  uint32_t threshold = P::kSumGroupBytes;
  uint32_t* raw = nullptr;      // [(kNC + 1) * blocks(cap)] the counts
  uint32_t* scanned = nullptr;  // ... their exclusive sums
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  gpk::Workspace ws;

  size_t cells() const { return (size_t)(P::kNC + 1) * ((cap + kBlk - 1) / kBlk); }
  void carve() {  // every device array of the handle
    ws.take(raw, cells()), ws.take(scanned, cells());
    ws.take(tmp, tmp_bytes ? tmp_bytes : 4);
  }
};

template <typename P>
struct Launch {
  PassHandle<P>* h;
  PassArgs<P> a;
  hipStream_t s;
};

template <typename P>
int launch_step(const gpk::DevTables* tab, void* arg) {
  Launch<P>& l = *static_cast<Launch<P>*>(arg);
  PassHandle<P>* h = l.h;
  PassArgs<P>& a = l.a;
  a.tab = tab;
  hipStream_t s = l.s;
  const size_t cells = (size_t)(P::kNC + 1) * a.nblocks;
  a.block_counts = h->raw;
  hipLaunchKernelGGL(classify_kernel<P>, dim3(a.nblocks), dim3(kBlk), 0, s, a);
  size_t tb = h->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(h->tmp, tb, h->raw, h->scanned, (int)cells, s) != hipSuccess) return GPK_EHIP;
  hipLaunchKernelGGL(finish_kernel<P::kNC>, dim3(1), dim3(64), 0, s, h->raw, h->scanned, a.nblocks, a.out.class_start,
                     a.out.counts);
  a.block_counts = h->scanned;
  hipLaunchKernelGGL(scatter_kernel<P>, dim3(a.nblocks), dim3(kBlk), 0, s, a);
  if (a.flags & P::kSumFlag) {
    const uint64_t want16 = (a.n + kBlk / 16 - 1) / (kBlk / 16), want64 = (a.n + kBlk - 1) / kBlk;
    const SumArgs<P> sa{a.data, a.offsets, a.caplens, a.records, a.layouts, a.out, h->threshold};
    hipLaunchKernelGGL(sum16_kernel<P>, dim3((unsigned)(want16 < 4096 ? want16 : 4096)), dim3(kBlk), 0, s, sa);
    hipLaunchKernelGGL(sum64_kernel<P>, dim3((unsigned)(want64 < 4096 ? want64 : 4096)), dim3(kBlk), 0, s, sa);
  }
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

template <typename P>
bool bad_args(const gpk_parser* p, const gpk_batch* b, const gpk_results* r, uint32_t kinds, uint32_t flags,
              const typename P::Out* o) {
  if (!p || !b || !r || !o || !o->class_start || !o->counts) return true;
  if (kinds == 0 || (kinds & ~P::kAll) || (flags & ~P::kSumFlag)) return true;
  if (b->n >= (1ull << 32)) return true;
  if (b->n && (!b->data || !b->offsets || !b->caplens || !r->records || !r->layouts || !o->verdict || !o->index ||
               P::missing(*o)))
    return true;
  return ((uintptr_t)P::entry(*o, 0) & 7) != 0;
}

// max_packets < limit; H: the public handle struct
template <typename H>
int pass_create(H** out, int device, uint64_t max_packets, uint64_t limit) {
  if (const int rc = gpk::check_create(out, device, max_packets, limit)) return rc;
  gpk::DeviceScope dscope(device);  // the caller's device is restored on return
  if (dscope.err != hipSuccess) return GPK_EHIP;
  H* h = new (std::nothrow) H();
  if (!h) return GPK_ENOMEM;
  h->device = device;
  h->cap = max_packets;
  const bool ok = hipcub::DeviceScan::ExclusiveSum(nullptr, h->tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                   (int)h->cells()) == hipSuccess;
  h->carve();
  if (!ok || !h->ws.alloc()) {
    delete h;
    return GPK_ENOMEM;
  }
  h->carve();
  *out = h;
  return GPK_OK;
}

template <typename H>
int pass_destroy(H* h) {
  if (!h) return GPK_EINVAL;
  gpk::DeviceScope dscope(h->device);
  (void)hipDeviceSynchronize();
  h->ws.release();
  delete h;
  return GPK_OK;
}

template <typename H>
int pass_set_sum_threshold(H* h, uint32_t bytes) {
  if (!h) return GPK_EINVAL;
  h->threshold = bytes;
  return GPK_OK;
}

template <typename H, typename P = typename H::Pass>
int pass_batch(H* h, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
               uint32_t flags, const typename P::Out* o, void* stream) {
  if (!h || !ctx || bad_args<P>(parser, b, r, kinds, flags, o)) return GPK_EINVAL;
  if (b->n > h->cap || ((uintptr_t)b->data & 15)) return GPK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  gpk::DeviceScope dscope(h->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (hipMemsetAsync(o->counts, 0, 8 * 4, s) != hipSuccess ||
      hipMemsetAsync(o->class_start, 0, (P::kNC + 1) * 4, s) != hipSuccess)
    return GPK_EHIP;
  if (b->n == 0) return GPK_OK;
  Launch<P> l{h, PassArgs<P>{b->data, b->offsets, b->caplens, r->records, r->layouts, nullptr, b->n, kinds, flags,
                             (uint32_t)((b->n + kBlk - 1) / kBlk), h->raw, *o},
              s};
  return gpk_with_device_tables(ctx, parser, stream, launch_step<P>, &l);
}

// the sum step's words on the host: big-endian 16-bit words, an odd last byte as a high byte
inline uint32_t host_words(const uint8_t* d, uint32_t len) {
  uint32_t s = 0;
  for (uint32_t k = 0; k + 1 < len; k += 2) s += (uint32_t)d[k] << 8 | d[k + 1];
  if (len & 1) s += (uint32_t)d[len - 1] << 8;
  return s;
}

// The pass on the calling thread: count, prefix, then a second pass that stores
// entry j and sums it in place, as the device's steps 3 and 4 do.
template <typename P>
int pass_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds, uint32_t flags,
                    const typename P::Out* o) {
  constexpr int kNC = P::kNC;
  if (bad_args<P>(parser, b, r, kinds, flags, o)) return GPK_EINVAL;
  const uint64_t n = b->n;
  const PassArgs<P> a{b->data, b->offsets, b->caplens, r->records, r->layouts, gpk_parser_tables(parser),
                      n, kinds, flags, 0, nullptr, *o};
  const SumArgs<P> sa{a.data, a.offsets, a.caplens, a.records, a.layouts, a.out, 0};
  uint32_t cnt[kNC] = {0}, sums = 0;
  int8_t* cls = n ? new (std::nothrow) int8_t[n] : nullptr;
  if (n && !cls) return GPK_ENOMEM;
  typename P::Rec rec;
  for (uint64_t i = 0; i < n; i++) {
    cls[i] = (int8_t)P::decode(a, i, rec);
    if (cls[i] >= 0) cnt[cls[i]]++;
  }
  uint32_t pos[kNC];
  o->class_start[0] = 0;
  for (int c = 0; c < kNC; c++) {
    pos[c] = o->class_start[c];
    o->class_start[c + 1] = o->class_start[c] + cnt[c];
  }
  for (uint64_t i = 0; i < n; i++) {
    if (cls[i] < 0) {
      o->verdict[i] = cls[i];
      continue;
    }
    P::decode(a, i, rec);
    const uint32_t j = pos[cls[i]]++;
    o->verdict[i] = (int32_t)j;
    o->index[j] = (uint32_t)i;
    P::emit(a, i, j, rec);
    if ((flags & P::kSumFlag) && P::wants_sum(rec)) {
      typename P::Packed* e = P::entry(*o, j);
      const uint32_t len = P::entry_len(*e);
      P::verdict(e, host_words(b->data + b->offsets[i] + e->hdr_off, len), P::start(sa, e, (uint32_t)i, len, 0));
      sums++;
    }
  }
  delete[] cls;
  o->counts[0] = o->class_start[kNC];
  for (int c = 0; c < kNC; c++) o->counts[1 + c] = cnt[c];
  for (int k = 1 + kNC; k < 8; k++) o->counts[k] = k == 1 + kNC ? sums : 0;
  return GPK_OK;
}

}  // namespace
