// gpk_tunnel.hip — one tunnel level peeled off a decoded batch
// (include/gpk_tunnel.h).
//
//   1. classify_kernel  one lane per packet: the rules of gpk_tunnel_rules.h
//                       give the packet's class; per 256-packet block the six
//                       class counts and the number of GRE sums to compute,
//                       stored row-major
//   2. exclusive scan   of the [7][blocks] counts: where each block's packets
//                       of each class start in the compact list (and, from the
//                       last row, how many sums there are: no atomic counts them)
//   3. scatter_kernel   one lane per packet again: its rank among the block's
//                       packets of its class (ballots, no atomics: the order is
//                       class, then packet index), then verdict, index, inner
//                       slice and the gpk_tunnel record at that position
//   4. gre_sum16/64     16 or 64 lanes per GRE entry with the C bit: the 16-bit
//                       one's-complement words of Contents‖Payload summed mod
//                       2^32 from 16-byte chunks, folded once
// The header decode runs twice (steps 1 and 3) instead of parking 72-byte
// records in a workspace: the header bytes are in cache, a record is not.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/gpk_tunnel.h"
#include "gpk_devguard.h"
#include "gpk_slice_sum.h"
#include "gpk_tunnel_rules.h"

// gpk_host.cpp (library-internal): the parser's tables in host memory, and a
// step enqueued on `stream` with their device copy (kept until it completes)
extern "C" __attribute__((visibility("hidden"))) const gpk::DevTables* gpk_parser_tables(const gpk_parser* p);
extern "C" __attribute__((visibility("hidden"))) int gpk_with_device_tables(
    gpk_ctx* c, const gpk_parser* p, void* stream, int (*step)(const gpk::DevTables*, void*), void* arg);

namespace {

constexpr int kBlk = 256;
constexpr int kNC = GPK_TUN_NCLASS;
constexpr int kRows = kNC + 1;  // the class counts, then the GRE sums to compute

struct PeelArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const gpk_record* records;
  const gpk_layout* layouts;
  const gpk::DevTables* tab;
  uint64_t n;
  uint32_t kinds, flags, nblocks;
  uint32_t* block_counts;  // [kRows][nblocks] row-major: the counts (classify), their exclusive sums (scatter)
  gpk_tunnels out;
};

__device__ __forceinline__ int peel_packet(const PeelArgs& a, uint64_t i, gpk::tun::Tun& t) {
  return gpk::tun::peel(a.tab, a.kinds, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], t);
}

__global__ void __launch_bounds__(kBlk) classify_kernel(PeelArgs a) {
  __shared__ uint32_t cnt[kRows];
  if (threadIdx.x < kRows) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  int cls = GPK_TUN_NONE;
  bool sum = false;
  if (i < a.n) {
    gpk::tun::Tun t;
    cls = peel_packet(a, i, t);
    sum = cls >= 0 && (a.flags & GPK_TUN_GRE_CSUM) && gpk::tun::wants_sum(t);
  }
#pragma unroll
  for (int c = 0; c < kRows; c++) {
    const uint64_t m = __ballot(c < kNC ? cls == c : sum);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&cnt[c], (uint32_t)__popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < kRows) a.block_counts[(size_t)threadIdx.x * a.nblocks + blockIdx.x] = cnt[threadIdx.x];
}

__global__ void finish_kernel(const uint32_t* raw, const uint32_t* scanned, uint32_t nblocks, uint32_t* class_start,
                              uint32_t* counts) {
  // scanned: exclusive sums of the row-major counts raw; a row's start is the total of the rows before it
  if (threadIdx.x == 0) {
    const size_t last = (size_t)kRows * nblocks - 1;
    for (int c = 0; c <= kNC; c++) class_start[c] = scanned[(size_t)c * nblocks];
    counts[0] = class_start[kNC];
    for (int c = 0; c < kNC; c++) counts[1 + c] = class_start[c + 1] - class_start[c];
    counts[7] = scanned[last] + raw[last] - class_start[kNC];
  }
}

__global__ void __launch_bounds__(kBlk) scatter_kernel(PeelArgs a) {
  __shared__ uint32_t wave_cnt[kBlk / 64][kNC];
  const uint64_t i = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int cls = GPK_TUN_NONE;
  gpk::tun::Tun t;
  if (i < a.n) cls = peel_packet(a, i, t);
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
  if ((a.flags & GPK_TUN_GRE_CSUM) && t.kind == GPK_TUN_GRE && !t.err && !gpk::tun::wants_sum(t))
    t.status |= GPK_TUN_ST_VALID;  // !ChecksumPresent: Valid without a sum (gre.go:246)
  a.out.verdict[i] = (int32_t)pos;
  a.out.index[pos] = (uint32_t)i;
  a.out.in_offsets[pos] = a.offsets[i] + t.inner_off;
  a.out.in_caplens[pos] = t.inner_len;
  gpk::tun::tun_store(&a.out.tunnels[pos], t);
}

using gpk::slice_sum;  // gpk_slice_sum.h: the sum body shared with gpk_control.hip

__device__ __forceinline__ void store_verdict(gpk_tunnel* t, uint32_t sum) {
  const uint32_t existing = t->gre_checksum, correct = gpk::tun::gre_correct(sum, existing);
  t->gre_correct = (uint16_t)correct;
  t->status = (uint8_t)(t->status | gpk::tun::gre_status(correct, existing));
}

// slices below the threshold: 16 lanes per entry, four entries per wave
__global__ void __launch_bounds__(kBlk) gre_sum16_kernel(const uint8_t* data, const uint64_t* offsets,
                                                         const gpk_tunnels out, uint32_t threshold) {
  constexpr int G = 16;
  const uint32_t m = out.counts[0];
  const uint32_t gl = threadIdx.x & (G - 1);
  const uint32_t groups = gridDim.x * (kBlk / G);
  for (uint32_t j = blockIdx.x * (kBlk / G) + threadIdx.x / G; j < m; j += groups) {
    gpk_tunnel* t = &out.tunnels[j];
    if (t->kind != GPK_TUN_GRE || t->err || !(t->raw0 & 0x80)) continue;  // gpk::tun::wants_sum
    const uint32_t len = t->contents_len + t->inner_len;
    if (len >= threshold) continue;
    const uint64_t lo = offsets[out.index[j]] + t->hdr_off;
    const uint32_t s = slice_sum<G>(data, lo, lo + len, gl);
    if (gl == 0) store_verdict(t, s);
  }
}

// slices from the threshold on: a wave looks at 64 entries, one per lane, and
// then sums each of the few long ones with all its lanes
__global__ void __launch_bounds__(kBlk) gre_sum64_kernel(const uint8_t* data, const uint64_t* offsets,
                                                         const gpk_tunnels out, uint32_t threshold) {
  const uint32_t m = out.counts[0];
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlk / 64);
  for (uint64_t base = ((uint64_t)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6)) * 64; base < m; base += waves * 64) {
    const uint64_t j = base + lane;
    uint32_t len = 0, lo_l = 0, lo_h = 0;
    bool big = false;
    if (j < m) {
      const gpk_tunnel* t = &out.tunnels[j];
      if (t->kind == GPK_TUN_GRE && !t->err && (t->raw0 & 0x80)) {
        len = t->contents_len + t->inner_len;
        big = len >= threshold;
        if (big) {
          const uint64_t lo = offsets[out.index[j]] + t->hdr_off;
          lo_l = (uint32_t)lo;
          lo_h = (uint32_t)(lo >> 32);
        }
      }
    }
    for (uint64_t todo = __ballot(big); todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const uint64_t lo = (uint64_t)(uint32_t)__shfl((int)lo_h, src) << 32 | (uint32_t)__shfl((int)lo_l, src);
      const uint32_t n = (uint32_t)__shfl((int)len, src);
      const uint32_t s = slice_sum<64>(data, lo, lo + n, lane);
      if (lane == 0) store_verdict(&out.tunnels[base + src], s);
    }
  }
}

}  // namespace

struct gpk_tunneler {
  int device = 0;
  uint64_t cap = 0;
  uint32_t threshold = GPK_TUN_SUM_GROUP_BYTES;
  uint32_t* block_counts = nullptr;  // 2 x [kRows * blocks(cap)]: the counts, their exclusive sums
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
};

namespace {
struct Launch {
  gpk_tunneler* t;
  PeelArgs a;
  hipStream_t s;
};

int launch_step(const gpk::DevTables* tab, void* arg) {
  Launch& l = *static_cast<Launch*>(arg);
  gpk_tunneler* t = l.t;
  PeelArgs& a = l.a;
  a.tab = tab;
  hipStream_t s = l.s;
  const size_t cells = (size_t)kRows * a.nblocks;
  hipLaunchKernelGGL(classify_kernel, dim3(a.nblocks), dim3(kBlk), 0, s, a);
  uint32_t* raw = a.block_counts;
  uint32_t* scanned = t->block_counts + (size_t)kRows * ((t->cap + kBlk - 1) / kBlk);
  size_t tb = t->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(t->tmp, tb, raw, scanned, (int)cells, s) != hipSuccess) return GPK_EHIP;
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, s, raw, scanned, a.nblocks, a.out.class_start, a.out.counts);
  a.block_counts = scanned;
  hipLaunchKernelGGL(scatter_kernel, dim3(a.nblocks), dim3(kBlk), 0, s, a);
  if (a.flags & GPK_TUN_GRE_CSUM) {
    const uint64_t want16 = (a.n + kBlk / 16 - 1) / (kBlk / 16), want64 = (a.n + kBlk - 1) / kBlk;
    hipLaunchKernelGGL(gre_sum16_kernel, dim3((unsigned)(want16 < 4096 ? want16 : 4096)), dim3(kBlk), 0, s, a.data,
                       a.offsets, a.out, t->threshold);
    hipLaunchKernelGGL(gre_sum64_kernel, dim3((unsigned)(want64 < 4096 ? want64 : 4096)), dim3(kBlk), 0, s, a.data,
                       a.offsets, a.out, t->threshold);
  }
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

bool bad_args(const gpk_parser* p, const gpk_batch* b, const gpk_results* r, uint32_t kinds, uint32_t flags,
              const gpk_tunnels* o) {
  if (!p || !b || !r || !o || !o->class_start || !o->counts) return true;
  if (kinds == 0 || (kinds & ~GPK_TUN_ALL) || (flags & ~GPK_TUN_GRE_CSUM)) return true;
  if (b->n >= (1ull << 32)) return true;
  if (b->n && (!b->data || !b->offsets || !b->caplens || !r->records || !r->layouts || !o->verdict || !o->index ||
               !o->in_offsets || !o->in_caplens || !o->tunnels))
    return true;
  return ((uintptr_t)o->tunnels & 7) != 0;
}
}  // namespace

extern "C" int gpk_tunneler_create(gpk_tunneler** out, int device, uint64_t max_packets) {
  if (!out || max_packets == 0 || max_packets >= (1ull << 32)) return GPK_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return GPK_ENODEV;
  gpk::DeviceScope dscope(device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  gpk_tunneler* t = new (std::nothrow) gpk_tunneler();
  if (!t) return GPK_ENOMEM;
  t->device = device;
  t->cap = max_packets;
  const size_t cells = (size_t)kRows * ((max_packets + kBlk - 1) / kBlk);
  bool ok = hipcub::DeviceScan::ExclusiveSum(nullptr, t->tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)cells) ==
            hipSuccess;
  ok = ok && hipMalloc((void**)&t->block_counts, 2 * cells * 4) == hipSuccess &&
       hipMalloc(&t->tmp, t->tmp_bytes ? t->tmp_bytes : 4) == hipSuccess;
  if (!ok) {
    if (t->block_counts) (void)hipFree(t->block_counts);
    if (t->tmp) (void)hipFree(t->tmp);
    delete t;
    return GPK_ENOMEM;
  }
  *out = t;
  return GPK_OK;
}

extern "C" int gpk_tunneler_destroy(gpk_tunneler* t) {
  if (!t) return GPK_EINVAL;
  gpk::DeviceScope dscope(t->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(t->block_counts);
  (void)hipFree(t->tmp);
  delete t;
  return GPK_OK;
}

extern "C" int gpk_tunneler_set_sum_threshold(gpk_tunneler* t, uint32_t bytes) {
  if (!t) return GPK_EINVAL;
  t->threshold = bytes;
  return GPK_OK;
}

extern "C" int gpk_tunnel_batch(gpk_tunneler* t, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                                const gpk_results* r, uint32_t kinds, uint32_t flags, const gpk_tunnels* o,
                                void* stream) {
  if (!t || !ctx || bad_args(parser, b, r, kinds, flags, o)) return GPK_EINVAL;
  if (b->n > t->cap || ((uintptr_t)b->data & 15)) return GPK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  gpk::DeviceScope dscope(t->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (hipMemsetAsync(o->counts, 0, 8 * 4, s) != hipSuccess || hipMemsetAsync(o->class_start, 0, 7 * 4, s) != hipSuccess)
    return GPK_EHIP;
  if (b->n == 0) return GPK_OK;
  Launch l{t, PeelArgs{b->data, b->offsets, b->caplens, r->records, r->layouts, nullptr, b->n, kinds, flags,
                       (uint32_t)((b->n + kBlk - 1) / kBlk), t->block_counts, *o},
           s};
  return gpk_with_device_tables(ctx, parser, stream, launch_step, &l);
}

extern "C" int gpk_tunnel_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                     uint32_t flags, const gpk_tunnels* o) {
  if (bad_args(parser, b, r, kinds, flags, o)) return GPK_EINVAL;
  const gpk::DevTables* T = gpk_parser_tables(parser);
  const uint64_t n = b->n;
  uint32_t cnt[kNC] = {0}, sums = 0;
  int8_t* cls = n ? new (std::nothrow) int8_t[n] : nullptr;
  if (n && !cls) return GPK_ENOMEM;
  gpk::tun::Tun t;
  for (uint64_t i = 0; i < n; i++) {
    cls[i] = (int8_t)gpk::tun::peel(T, kinds, b->data + b->offsets[i], b->caplens[i], r->records[i], r->layouts[i], t);
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
    const uint8_t* p = b->data + b->offsets[i];
    gpk::tun::peel(T, kinds, p, b->caplens[i], r->records[i], r->layouts[i], t);
    if ((flags & GPK_TUN_GRE_CSUM) && t.kind == GPK_TUN_GRE && !t.err) {
      if (gpk::tun::wants_sum(t)) {
        const uint8_t* d = p + t.hdr_off;
        const uint32_t len = t.contents_len + t.inner_len;
        uint32_t s = 0;
        for (uint32_t k = 0; k + 1 < len; k += 2) s += (uint32_t)d[k] << 8 | d[k + 1];
        if (len & 1) s += (uint32_t)d[len - 1] << 8;
        t.correct = gpk::tun::gre_correct(s, t.checksum);
        t.status |= gpk::tun::gre_status(t.correct, t.checksum);
        sums++;
      } else {
        t.status |= GPK_TUN_ST_VALID;
      }
    }
    const uint32_t j = pos[cls[i]]++;
    o->verdict[i] = (int32_t)j;
    o->index[j] = (uint32_t)i;
    o->in_offsets[j] = b->offsets[i] + t.inner_off;
    o->in_caplens[j] = t.inner_len;
    gpk::tun::tun_store(&o->tunnels[j], t);
  }
  delete[] cls;
  o->counts[0] = o->class_start[kNC];
  for (int c = 0; c < kNC; c++) o->counts[1 + c] = cnt[c];
  o->counts[7] = sums;
  return GPK_OK;
}

extern "C" int gpk_tunnel_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  const char* s = nullptr;
  switch (err) {
    case 0: s = ""; break;
    case GPK_TUN_ERR_VXLAN_SMALL: s = "vxlan packet too small"; break;
    case GPK_TUN_ERR_GRE_SMALL: s = "GRE packet too small"; break;
    case GPK_TUN_ERR_GRE_TRUNCATED: s = "GRE packet truncated"; break;
    case GPK_TUN_ERR_GENEVE_OPT_SHORT:
    case GPK_TUN_ERR_GENEVE_OPT_LEN: s = "geneve option too small"; break;
    case GPK_TUN_ERR_GENEVE_SHORT:
    case GPK_TUN_ERR_GENEVE_OPTS_SHORT: s = "geneve packet too short"; break;
    case GPK_ERR_PANIC_INDEX:
    case GPK_ERR_PANIC_SLICE_ACAP:
    case GPK_ERR_PANIC_SLICE_B: return gpk_format_error(err, a0, a1, buf, cap);
    default: return GPK_EINVAL;
  }
  const int n = snprintf(buf, cap, "%s", s);
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
