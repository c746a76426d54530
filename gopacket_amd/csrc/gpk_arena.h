// gpk_arena.h — the second stage of a pass of gpk_postpass.h whose result has a
// variable length (library-internal). gpk_dns.hip, gpk_tls.hip,
// gpk_ndp.hip and gpk_svc.hip are its users: each supplies a policy A, its
// extern "C" entries and its error texts.
//
// The pass leaves a compact list of m fixed-size entries, each with the sizes
// of what its message holds (resource records and name bytes, say). Then
//   1. exclusive scan  of those sizes over the list: the totals in front of
//                      each message, so where its ranges of the caller's arenas
//                      start
//   2. emit_kernel     one lane per message: stores those starts in the entry
//                      and, when the whole range fits every capacity, walks the
//                      message again in store form; otherwise the entry is
//                      marked A::kDropped. The last entry reports what the batch
//                      needs: counts[3] is set when a capacity is too small,
//                      counts[4..] hold the 64-bit totals
//
// A policy A derives from NoSum and supplies what gpk_postpass.h asks of a
// policy (Rec, Packed, Out, kNC, kNone, kAll, decode, emit, missing, entry), and
//   kCounts, kDropped  the words of counts[] (8, or more: the pass zeroes the
//                      first eight, this stage the rest); the status bit of a
//                      message that did not fit
//   Tot, own(packed), add(t, u)
//                      the totals: a POD of uint64_t members whose zero is
//                      Tot{}, or uint64_t itself where there is one; those of
//                      one entry; their sum                      (host + device)
//   fits(out, t, end)  whether the range from t to end lies inside every
//                      capacity. A pass whose messages with nothing to store
//                      are never dropped lets an empty range fit  (host + device)
//   report(counts, end) counts[4..] from the batch's totals      (host + device)
//   place(packed, t)   store the starts in the entry             (host + device)
//   walk(a, j, packed, t, end)
//                      the message of entry j again, storing from t on (to end)
//                                                                (host + device)
//   bad_out(out, kinds) whether the arenas or the kinds are invalid
#pragma once
#include <cstdio>

#include "gpk_postpass.h"
#include "gpk_tunnel_rules.h"  // GPK_HD; every pass's rules build on it

namespace {

// the sum hooks of a pass that sums nothing: those kernels never launch
struct NoSum {
  static constexpr uint32_t kSumFlag = 0, kSumGroupBytes = 0;
  template <typename R>
  static GPK_HD bool wants_sum(const R&) {
    return false;
  }
  template <typename K>
  static GPK_HD bool entry_wants_sum(const K&) {
    return false;
  }
  template <typename K>
  static GPK_HD uint32_t entry_len(const K&) {
    return 0;
  }
  template <typename S, typename K>
  static GPK_HD uint32_t start(const S&, const K*, uint32_t, uint32_t, uint32_t) {
    return 0;
  }
  template <typename K>
  static GPK_HD void verdict(K*, uint32_t, uint32_t) {}
};

GPK_HD void put64(uint32_t* c, uint64_t v) { c[0] = (uint32_t)v, c[1] = (uint32_t)(v >> 32); }

template <typename A>
struct TotAdd {
  __host__ __device__ typename A::Tot operator()(const typename A::Tot& a, const typename A::Tot& b) const {
    return A::add(a, b);
  }
};
template <typename A>
struct TotOf {  // of entry j; nothing past m
  const typename A::Packed* records;
  const uint32_t* counts;
  __host__ __device__ typename A::Tot operator()(uint32_t j) const {
    return j < counts[0] ? A::own(records[j]) : typename A::Tot{};
  }
};
template <typename A>
using TotIn = hipcub::TransformInputIterator<typename A::Tot, TotOf<A>, hipcub::CountingInputIterator<uint32_t>>;

// the scan, or with tmp == nullptr its size query
template <typename A>
hipError_t scan_totals(void* tmp, size_t& tmp_bytes, const typename A::Out& out, typename A::Tot* starts, uint64_t n,
                       hipStream_t s) {
  const TotIn<A> in(hipcub::CountingInputIterator<uint32_t>(0), TotOf<A>{A::entry(out, 0), out.counts});
  return hipcub::DeviceScan::ExclusiveScan(tmp, tmp_bytes, in, starts, TotAdd<A>(), typename A::Tot{}, (int)n, s);
}

template <typename A>
struct EmitArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const typename A::Tot* starts;
  typename A::Out out;
};

// Entry j (< m) of the compact list, t: the totals in front of it. The last
// entry also reports what the batch needs (the batch as one range from zero).
// t comes by value and err is read with the sizes, in front of the report's
// stores: the lane then waits once for its first loads (starts[j], the sizes,
// err), not for one after the other.
template <typename A>
GPK_HD void emit_one(const EmitArgs<A>& a, uint32_t j, uint32_t m, const typename A::Tot t) {
  typename A::Packed* r = A::entry(a.out, j);
  const typename A::Tot end = A::add(t, A::own(*r));
  const auto err = r->err;
  if (j == m - 1) {
    a.out.counts[3] = !A::fits(a.out, typename A::Tot{}, end);
    A::report(a.out.counts, end);
  }
  if (err) return;
  A::place(r, t);
  if (!A::fits(a.out, t, end)) {
    r->status |= A::kDropped;
    return;
  }
  A::walk(a, j, r, t, end);
}

template <typename A>
__global__ void __launch_bounds__(kBlk) emit_kernel(const EmitArgs<A> a) {
  const uint32_t m = a.out.counts[0];
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < m) emit_one<A>(a, (uint32_t)j, m, a.starts[j]);
}

// ---- the handle: the four decoders derive from it

template <typename A>
struct ArenaHandle : PassHandle<A> {
  typename A::Tot* starts = nullptr;  // [cap]
  uint8_t* tmp2 = nullptr;
  size_t tmp2_bytes = 0;
  void carve() {
    PassHandle<A>::carve();
    if (!tmp2_bytes && scan_totals<A>(nullptr, tmp2_bytes, typename A::Out{}, nullptr, this->cap, 0) != hipSuccess)
      tmp2_bytes = 0;
    this->ws.take(starts, this->cap);
    this->ws.take(tmp2, tmp2_bytes ? tmp2_bytes : 4);
  }
};

template <typename H>
int arena_create(H** out, int device, uint64_t max_packets) {
  if (const int rc = pass_create(out, device, max_packets, 1ull << 28)) return rc;
  if ((*out)->tmp2_bytes == 0) {  // the second scan's size query failed in carve(): as pass_create reports the first
    pass_destroy(*out);
    *out = nullptr;
    return GPK_ENOMEM;
  }
  return GPK_OK;
}

template <typename H, typename A = typename H::Pass>
int arena_batch(H* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                const typename A::Out* o, void* stream) {
  if (!d || A::bad_out(o, kinds)) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  hipStream_t s = (hipStream_t)stream;
  if constexpr (A::kCounts > 8) {  // the pass zeroes the first eight; an invalid call writes nothing
    if (!ctx || bad_args<A>(parser, b, r, kinds, 0, o)) return GPK_EINVAL;
    if (hipMemsetAsync(o->counts + 8, 0, (A::kCounts - 8) * 4, s) != hipSuccess) return GPK_EHIP;
  }
  if (const int rc = pass_batch(d, ctx, parser, b, r, kinds, 0, o, stream)) return rc;
  if (b->n == 0) return GPK_OK;
  size_t tb = d->tmp2_bytes;
  if (scan_totals<A>(d->tmp2, tb, *o, d->starts, b->n, s) != hipSuccess) return GPK_EHIP;
  const EmitArgs<A> ea{b->data, b->offsets, b->caplens, d->starts, *o};
  hipLaunchKernelGGL(emit_kernel<A>, dim3((unsigned)((b->n + kBlk - 1) / kBlk)), dim3(kBlk), 0, s, ea);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

// The stage on the calling thread: a running total in place of the scan.
template <typename A>
int arena_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                     const typename A::Out* o) {
  if (A::bad_out(o, kinds)) return GPK_EINVAL;
  if (const int rc = pass_batch_host<A>(parser, b, r, kinds, 0, o)) return rc;
  for (int k = 8; k < A::kCounts; k++) o->counts[k] = 0;
  const EmitArgs<A> ea{b->data, b->offsets, b->caplens, nullptr, *o};
  const uint32_t m = o->counts[0];
  typename A::Tot t{};
  for (uint32_t j = 0; j < m; j++) {
    const typename A::Tot own = A::own(*A::entry(*o, j));
    emit_one<A>(ea, j, m, t);
    t = A::add(t, own);
  }
  return GPK_OK;
}

// The tail of a gpk_*_format_error: text[err - first] for first <= err < end,
// the empty string for 0; a text takes none, one or both arguments.
inline int format_text(const char* const* text, unsigned first, unsigned end, unsigned err, uint32_t a0, uint32_t a1,
                       char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  int n;
  if (err == 0) n = snprintf(buf, cap, "%s", "");
  else if (err < first || err >= end) return GPK_EINVAL;
  else n = snprintf(buf, cap, text[err - first], a0, a1);
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}

}  // namespace
