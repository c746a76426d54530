// gpk_control.hip — the ICMPv4, ICMPv6 (+Echo) and ARP layers at the end of a
// decoded batch (include/gpk_control.h). The shape is
// gpk_tunnel.hip's:
//
//   1. classify_kernel  one lane per packet: the rules of gpk_control_rules.h
//                       give the packet's class; per 256-packet block the four
//                       class counts and the number of sums to make, row-major
//   2. exclusive scan   of the [5][blocks] counts, then finish_kernel
//   3. scatter_kernel   one lane per packet again: its rank among the block's
//                       packets of its class (ballots, no atomics: the order is
//                       class, then packet index), then verdict, index and the
//                       gpk_control record at that position. The decode runs a
//                       second time: the header bytes are in cache, a parked
//                       record would not be.
//   4. sum16/64         16 or 64 lanes per ICMPv4 / ICMPv6 entry: the words of
//                       Contents‖Payload summed mod 2^32 from 16-byte chunks
//                       (gpk_slice_sum.h, the GRE sum's body), plus ICMPv6's
//                       start value (16 lanes read the pseudo-header's address
//                       words, one each), folded once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/gpk_control.h"
#include "gpk_control_rules.h"
#include "gpk_devguard.h"
#include "gpk_slice_sum.h"
#include "gpk_workspace.h"

// gpk_host.cpp (library-internal): the parser's tables in host memory, and a
// step enqueued on `stream` with their device copy (kept until it completes)
extern "C" __attribute__((visibility("hidden"))) const gpk::DevTables* gpk_parser_tables(const gpk_parser* p);
extern "C" __attribute__((visibility("hidden"))) int gpk_with_device_tables(
    gpk_ctx* c, const gpk_parser* p, void* stream, int (*step)(const gpk::DevTables*, void*), void* arg);

namespace {

using gpk::slice_sum;

constexpr int kBlk = 256;
constexpr int kNC = GPK_CTL_NCLASS;
constexpr int kRows = kNC + 1;  // the class counts, then the sums to make

struct CtlArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const gpk_record* records;
  const gpk_layout* layouts;
  const gpk::DevTables* tab;
  uint64_t n;
  uint32_t kinds, flags, nblocks;
  uint32_t* block_counts;  // [kRows][nblocks] row-major: the counts (classify), their exclusive sums (scatter)
  gpk_controls out;
};

__device__ __forceinline__ int control_packet(const CtlArgs& a, uint64_t i, gpk::ctl::Ctl& c) {
  return gpk::ctl::control(a.tab, a.kinds, a.flags, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], c);
}

__global__ void __launch_bounds__(kBlk) ctl_classify_kernel(CtlArgs a) {
  __shared__ uint32_t cnt[kRows];
  if (threadIdx.x < kRows) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  int cls = GPK_CTL_NONE;
  bool sum = false;
  if (i < a.n) {
    gpk::ctl::Ctl c;
    cls = control_packet(a, i, c);
    sum = cls >= 0 && (a.flags & GPK_CTL_CSUM) && gpk::ctl::wants_sum(c.kind, c.nlayers, c.status);
  }
#pragma unroll
  for (int r = 0; r < kRows; r++) {
    const uint64_t m = __ballot(r < kNC ? cls == r : sum);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&cnt[r], (uint32_t)__popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < kRows) a.block_counts[(size_t)threadIdx.x * a.nblocks + blockIdx.x] = cnt[threadIdx.x];
}

__global__ void ctl_finish_kernel(const uint32_t* raw, const uint32_t* scanned, uint32_t nblocks, uint32_t* class_start,
                                  uint32_t* counts) {
  // scanned: exclusive sums of the row-major counts raw; a row's start is the total of the rows before it
  if (threadIdx.x == 0) {
    const size_t last = (size_t)kRows * nblocks - 1;
    for (int c = 0; c <= kNC; c++) class_start[c] = scanned[(size_t)c * nblocks];
    counts[0] = class_start[kNC];
    for (int c = 0; c < kNC; c++) counts[1 + c] = class_start[c + 1] - class_start[c];
    counts[1 + kNC] = scanned[last] + raw[last] - class_start[kNC];
  }
}

__global__ void __launch_bounds__(kBlk) ctl_scatter_kernel(CtlArgs a) {
  __shared__ uint32_t wave_cnt[kBlk / 64][kNC];
  const uint64_t i = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int cls = GPK_CTL_NONE;
  gpk::ctl::Ctl c;
  if (i < a.n) cls = control_packet(a, i, c);
  uint32_t rank = 0;
#pragma unroll
  for (int r = 0; r < kNC; r++) {
    const uint64_t m = __ballot(cls == r);
    if (lane == 0) wave_cnt[wave][r] = (uint32_t)__popcll(m);
    if (cls == r) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1));
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
  gpk::ctl::ctl_store(&a.out.records[pos], c);
}

struct SumArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const gpk_record* records;
  const gpk_layout* layouts;
  gpk_controls out;
  uint32_t threshold;
};

// An ICMPv6 entry's start value, by the first 16 lanes of its group (gl < 16): the
// pseudo-header's 4 or 16 address words, one per lane (one line per group, where a
// lane of the scatter would touch a line per packet for every word), reduced over 16
// lanes; 0 for ICMPv4. Every lane of the group returns the value.
__device__ __forceinline__ uint32_t start_of(const SumArgs& a, const gpk_control* r, uint32_t pkt, uint32_t len,
                                             uint32_t gl) {
  if (r->kind != GPK_CTL_ICMP6) return 0;
  gpk::ctl::Net net;
  if (!gpk::ctl::network_layer(a.caplens[pkt], a.records[pkt], a.layouts[pkt], net)) return 0;  // not reached: NONET
  uint32_t w = 0;
  if (2 * gl < net.bytes) w = gpk::ctl::be16(a.data + a.offsets[pkt] + net.off + 2 * gl);
#pragma unroll
  for (int d = 8; d > 0; d >>= 1) w += (uint32_t)__shfl_xor((int)w, d, 16);
  return gpk::ctl::start_value(w, len);
}

__device__ __forceinline__ void store_verdict(gpk_control* r, uint32_t sum, uint32_t start) {
  const uint32_t existing = r->checksum, correct = gpk::ctl::correct_of(sum + start, existing);
  r->sum_init = start;
  r->correct = (uint16_t)correct;
  r->status = (uint8_t)(r->status | gpk::ctl::sum_status(correct, existing));
}

// messages below the threshold: 16 lanes per entry, four entries per wave
__global__ void __launch_bounds__(kBlk) ctl_sum16_kernel(const SumArgs a) {
  constexpr int G = 16;
  const gpk_controls& out = a.out;
  const uint32_t m = out.counts[0];
  const uint32_t gl = threadIdx.x & (G - 1);
  const uint32_t groups = gridDim.x * (kBlk / G);
  for (uint32_t j = blockIdx.x * (kBlk / G) + threadIdx.x / G; j < m; j += groups) {
    gpk_control* r = &out.records[j];
    if (!gpk::ctl::wants_sum(r->kind, r->nlayers, r->status)) continue;
    const uint32_t len = r->contents_len + r->payload_len;
    if (len >= a.threshold) continue;
    const uint32_t pkt = out.index[j];
    const uint64_t lo = a.offsets[pkt] + r->hdr_off;
    const uint32_t start = start_of(a, r, pkt, len, gl);
    const uint32_t s = slice_sum<G>(a.data, lo, lo + len, gl);
    if (gl == 0) store_verdict(r, s, start);
  }
}

// messages from the threshold on: a wave looks at 64 entries, one per lane, and
// then sums each of the few long ones with all its lanes
__global__ void __launch_bounds__(kBlk) ctl_sum64_kernel(const SumArgs a) {
  const gpk_controls& out = a.out;
  const uint32_t m = out.counts[0];
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * (kBlk / 64);
  for (uint64_t base = ((uint64_t)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6)) * 64; base < m; base += waves * 64) {
    const uint64_t j = base + lane;
    uint32_t len = 0, lo_l = 0, lo_h = 0;
    bool big = false;
    if (j < m) {
      const gpk_control* r = &out.records[j];
      if (gpk::ctl::wants_sum(r->kind, r->nlayers, r->status)) {
        len = r->contents_len + r->payload_len;
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
      gpk_control* r = &out.records[base + src];
      const uint32_t start = start_of(a, r, out.index[base + src], n, lane & 15);
      const uint32_t s = slice_sum<64>(a.data, lo, lo + n, lane);
      if (lane == 0) store_verdict(r, s, start);
    }
  }
}

}  // namespace

struct gpk_controller {
  int device = 0;
  uint64_t cap = 0;
  uint32_t threshold = GPK_CTL_SUM_GROUP_BYTES;
  uint32_t* raw = nullptr;      // [kRows * blocks(cap)] the counts
  uint32_t* scanned = nullptr;  // ... their exclusive sums
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  gpk::Workspace ws;
};

namespace {

size_t cells_of(uint64_t n) { return (size_t)kRows * ((n + kBlk - 1) / kBlk); }

void carve(gpk_controller* c) {  // every device array of the handle
  c->ws.take(c->raw, cells_of(c->cap)), c->ws.take(c->scanned, cells_of(c->cap));
  c->ws.take(c->tmp, c->tmp_bytes ? c->tmp_bytes : 4);
}

struct Launch {
  gpk_controller* c;
  CtlArgs a;
  hipStream_t s;
};

int launch_step(const gpk::DevTables* tab, void* arg) {
  Launch& l = *static_cast<Launch*>(arg);
  gpk_controller* c = l.c;
  CtlArgs& a = l.a;
  a.tab = tab;
  hipStream_t s = l.s;
  const size_t cells = (size_t)kRows * a.nblocks;
  a.block_counts = c->raw;
  hipLaunchKernelGGL(ctl_classify_kernel, dim3(a.nblocks), dim3(kBlk), 0, s, a);
  size_t tb = c->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(c->tmp, tb, c->raw, c->scanned, (int)cells, s) != hipSuccess) return GPK_EHIP;
  hipLaunchKernelGGL(ctl_finish_kernel, dim3(1), dim3(64), 0, s, c->raw, c->scanned, a.nblocks, a.out.class_start,
                     a.out.counts);
  a.block_counts = c->scanned;
  hipLaunchKernelGGL(ctl_scatter_kernel, dim3(a.nblocks), dim3(kBlk), 0, s, a);
  if (a.flags & GPK_CTL_CSUM) {
    const uint64_t want16 = (a.n + kBlk / 16 - 1) / (kBlk / 16), want64 = (a.n + kBlk - 1) / kBlk;
    const SumArgs sa{a.data, a.offsets, a.caplens, a.records, a.layouts, a.out, c->threshold};
    hipLaunchKernelGGL(ctl_sum16_kernel, dim3((unsigned)(want16 < 4096 ? want16 : 4096)), dim3(kBlk), 0, s, sa);
    hipLaunchKernelGGL(ctl_sum64_kernel, dim3((unsigned)(want64 < 4096 ? want64 : 4096)), dim3(kBlk), 0, s, sa);
  }
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

bool bad_args(const gpk_parser* p, const gpk_batch* b, const gpk_results* r, uint32_t kinds, uint32_t flags,
              const gpk_controls* o) {
  if (!p || !b || !r || !o || !o->class_start || !o->counts) return true;
  if (kinds == 0 || (kinds & ~GPK_CTL_ALL) || (flags & ~GPK_CTL_CSUM)) return true;
  if (b->n >= (1ull << 32)) return true;
  if (b->n && (!b->data || !b->offsets || !b->caplens || !r->records || !r->layouts || !o->verdict || !o->index ||
               !o->records))
    return true;
  return ((uintptr_t)o->records & 7) != 0;
}
}  // namespace

extern "C" int gpk_controller_create(gpk_controller** out, int device, uint64_t max_packets) {
  if (const int rc = gpk::check_create(out, device, max_packets)) return rc;
  gpk::DeviceScope dscope(device);  // the caller's device is restored on return
  if (dscope.err != hipSuccess) return GPK_EHIP;
  gpk_controller* c = new (std::nothrow) gpk_controller();
  if (!c) return GPK_ENOMEM;
  c->device = device;
  c->cap = max_packets;
  const bool ok = hipcub::DeviceScan::ExclusiveSum(nullptr, c->tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                   (int)cells_of(max_packets)) == hipSuccess;
  carve(c);
  if (!ok || !c->ws.alloc()) {
    delete c;
    return GPK_ENOMEM;
  }
  carve(c);
  *out = c;
  return GPK_OK;
}

extern "C" int gpk_controller_destroy(gpk_controller* c) {
  if (!c) return GPK_EINVAL;
  gpk::DeviceScope dscope(c->device);
  (void)hipDeviceSynchronize();
  c->ws.release();
  delete c;
  return GPK_OK;
}

extern "C" int gpk_controller_set_sum_threshold(gpk_controller* c, uint32_t bytes) {
  if (!c) return GPK_EINVAL;
  c->threshold = bytes;
  return GPK_OK;
}

extern "C" int gpk_control_batch(gpk_controller* c, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                                 const gpk_results* r, uint32_t kinds, uint32_t flags, const gpk_controls* o,
                                 void* stream) {
  if (!c || !ctx || bad_args(parser, b, r, kinds, flags, o)) return GPK_EINVAL;
  if (b->n > c->cap || ((uintptr_t)b->data & 15)) return GPK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  gpk::DeviceScope dscope(c->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (hipMemsetAsync(o->counts, 0, 8 * 4, s) != hipSuccess ||
      hipMemsetAsync(o->class_start, 0, (kNC + 1) * 4, s) != hipSuccess)
    return GPK_EHIP;
  if (b->n == 0) return GPK_OK;
  Launch l{c, CtlArgs{b->data, b->offsets, b->caplens, r->records, r->layouts, nullptr, b->n, kinds, flags,
                      (uint32_t)((b->n + kBlk - 1) / kBlk), c->raw, *o},
           s};
  return gpk_with_device_tables(ctx, parser, stream, launch_step, &l);
}

extern "C" int gpk_control_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                      uint32_t flags, const gpk_controls* o) {
  if (bad_args(parser, b, r, kinds, flags, o)) return GPK_EINVAL;
  const gpk::DevTables* T = gpk_parser_tables(parser);
  const uint64_t n = b->n;
  uint32_t cnt[kNC] = {0}, sums = 0;
  int8_t* cls = n ? new (std::nothrow) int8_t[n] : nullptr;
  if (n && !cls) return GPK_ENOMEM;
  gpk::ctl::Ctl c;
  for (uint64_t i = 0; i < n; i++) {
    cls[i] = (int8_t)gpk::ctl::control(T, kinds, flags, b->data + b->offsets[i], b->caplens[i], r->records[i],
                                       r->layouts[i], c);
    if (cls[i] >= 0) cnt[cls[i]]++;
  }
  uint32_t pos[kNC];
  o->class_start[0] = 0;
  for (int k = 0; k < kNC; k++) {
    pos[k] = o->class_start[k];
    o->class_start[k + 1] = o->class_start[k] + cnt[k];
  }
  for (uint64_t i = 0; i < n; i++) {
    if (cls[i] < 0) {
      o->verdict[i] = cls[i];
      continue;
    }
    const uint8_t* p = b->data + b->offsets[i];
    gpk::ctl::control(T, kinds, flags, p, b->caplens[i], r->records[i], r->layouts[i], c);
    if ((flags & GPK_CTL_CSUM) && gpk::ctl::wants_sum(c.kind, c.nlayers, c.status)) {
      const uint8_t* d = p + c.hdr_off;
      const uint32_t len = c.contents_len + c.payload_len;
      gpk::ctl::Net net;
      if (c.kind == GPK_CTL_ICMP6 && gpk::ctl::network_layer(b->caplens[i], r->records[i], r->layouts[i], net)) {
        uint32_t w = 0;
        for (uint32_t q = 0; q < net.bytes; q += 2) w += gpk::ctl::be16(p + net.off + q);
        c.sum_init = gpk::ctl::start_value(w, len);
      }
      uint32_t s = c.sum_init;
      for (uint32_t k = 0; k + 1 < len; k += 2) s += (uint32_t)d[k] << 8 | d[k + 1];
      if (len & 1) s += (uint32_t)d[len - 1] << 8;
      c.correct = gpk::ctl::correct_of(s, c.checksum);
      c.status |= gpk::ctl::sum_status(c.correct, c.checksum);
      sums++;
    }
    const uint32_t j = pos[cls[i]]++;
    o->verdict[i] = (int32_t)j;
    o->index[j] = (uint32_t)i;
    gpk::ctl::ctl_store(&o->records[j], c);
  }
  delete[] cls;
  o->counts[0] = o->class_start[kNC];
  for (int k = 0; k < kNC; k++) o->counts[1 + k] = cnt[k];
  o->counts[1 + kNC] = sums;
  o->counts[6] = o->counts[7] = 0;
  return GPK_OK;
}

extern "C" int gpk_control_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  int n;
  switch (err) {
    case 0: n = snprintf(buf, cap, "%s", ""); break;
    case GPK_CTL_ERR_ICMP4_SHORT: n = snprintf(buf, cap, "ICMP layer less then 8 bytes for ICMPv4 packet"); break;
    case GPK_CTL_ERR_ICMP6_SHORT: n = snprintf(buf, cap, "ICMP layer less then 4 bytes for ICMPv6 packet"); break;
    case GPK_CTL_ERR_ECHO_SHORT: n = snprintf(buf, cap, "ICMP layer less then 4 bytes for ICMPv6 Echo"); break;
    case GPK_CTL_ERR_ARP_SHORT: n = snprintf(buf, cap, "ARP length %u too short", a0); break;
    case GPK_CTL_ERR_ARP_EXPECTED: n = snprintf(buf, cap, "ARP length %u too short, %u expected", a0, a1); break;
    default: return GPK_EINVAL;
  }
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
