// gpk_ndp.hip — the NDP and MLD messages behind ICMPv6 at the end of a decoded
// batch (include/gpk_ndp.h): the pass of gpk_postpass.h with the
// rules of gpk_ndp_rules.h (no sum), then what a variable-length result needs:
//   scan          exclusive sums of nentries over the compact list: where each
//                 message's entries start
//   emit_kernel   one lane per message: stores entry0 and, when the message's
//                 whole range fits entry_cap, walks again in emit form
#include <cstdio>

#include "../../include/gpk_ndp.h"
#include "gpk_ndp_rules.h"
#include "gpk_postpass.h"

namespace {

struct NdpPass {
  using Rec = gpk::ndp::Msg;
  using Packed = gpk_ndp;
  using Out = gpk_ndps;
  static constexpr int kNC = GPK_NDP_NCLASS, kNone = GPK_NDP_NONE;
  static constexpr uint32_t kAll = GPK_NDP_ALL, kSumFlag = 0, kSumGroupBytes = 0;  // no sum: those kernels never launch

  static GPK_HD int decode(const PassArgs<NdpPass>& a, uint64_t i, Rec& m) {
    return gpk::ndp::ndp(a.tab, a.kinds, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD bool wants_sum(const Rec&) { return false; }
  static GPK_HD void emit(const PassArgs<NdpPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::ndp::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }
  static GPK_HD bool entry_wants_sum(const Packed&) { return false; }
  static GPK_HD uint32_t entry_len(const Packed&) { return 0; }
  static GPK_HD uint32_t start(const SumArgs<NdpPass>&, const Packed*, uint32_t, uint32_t, uint32_t) { return 0; }
  static GPK_HD void verdict(Packed*, uint32_t, uint32_t) {}
};

struct CountOf {  // entries of message j; nothing past m
  const gpk_ndp* records;
  const uint32_t* counts;
  __host__ __device__ uint64_t operator()(uint32_t j) const { return j < counts[0] ? records[j].nentries : 0; }
};
using CountIn = hipcub::TransformInputIterator<uint64_t, CountOf, hipcub::CountingInputIterator<uint32_t>>;

struct EmitArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint64_t* starts;
  gpk_ndps out;
};

// Entry j (< m) of the compact list, t: the entries in front of it. The last
// one also reports what the batch needs.
GPK_HD void emit_one(const EmitArgs& a, uint32_t j, uint32_t m, uint64_t t) {
  gpk_ndp* r = &a.out.records[j];
  const uint32_t own = r->nentries;
  if (j == m - 1) {
    const uint64_t need = t + own;
    a.out.counts[3] = need > a.out.entry_cap;
    a.out.counts[4] = (uint32_t)need, a.out.counts[5] = (uint32_t)(need >> 32);
  }
  if (r->err) return;
  r->entry0 = t;
  if (own == 0) return;
  if (t + own > a.out.entry_cap) {
    r->status |= GPK_NDP_ST_DROPPED;
    return;
  }
  gpk::ndp::Msg msg;
  gpk::ndp::msg_init(msg, r->layer_type, r->hdr_off);
  gpk::ndp::walk<true>(a.data + a.offsets[a.out.index[j]] + r->hdr_off, r->len, msg, a.out.entries + t);
}

__global__ void __launch_bounds__(kBlk) emit_kernel(const EmitArgs a) {
  const uint32_t m = a.out.counts[0];
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < m) emit_one(a, (uint32_t)j, m, a.starts[j]);
}

bool bad_out(const gpk_ndps* o, uint32_t kinds) {
  return !o || ((uintptr_t)o->entries & 7) || (o->entry_cap && !o->entries) || kinds == GPK_NDP_ICMP6;
}

}  // namespace

struct gpk_ndp_decoder : PassHandle<NdpPass> {
  uint64_t* starts = nullptr;  // [cap]
  uint8_t* tmp2 = nullptr;
  size_t tmp2_bytes = 0;
  void carve() {
    PassHandle<NdpPass>::carve();
    if (!tmp2_bytes &&
        hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2_bytes,
                                         CountIn(hipcub::CountingInputIterator<uint32_t>(0), CountOf{nullptr, nullptr}),
                                         (uint64_t*)nullptr, (int)cap) != hipSuccess)
      tmp2_bytes = 0;
    ws.take(starts, cap);
    ws.take(tmp2, tmp2_bytes ? tmp2_bytes : 4);
  }
};

extern "C" int gpk_ndp_decoder_create(gpk_ndp_decoder** out, int device, uint64_t max_packets) {
  if (const int rc = pass_create(out, device, max_packets, 1ull << 28)) return rc;
  if ((*out)->tmp2_bytes == 0) {  // the second scan's size query failed in carve(): as pass_create reports the first
    pass_destroy(*out);
    *out = nullptr;
    return GPK_ENOMEM;
  }
  return GPK_OK;
}
extern "C" int gpk_ndp_decoder_destroy(gpk_ndp_decoder* d) { return pass_destroy(d); }

extern "C" int gpk_ndp_batch(gpk_ndp_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, uint32_t kinds, const gpk_ndps* o, void* stream) {
  if (!d || bad_out(o, kinds)) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (const int rc = pass_batch(d, ctx, parser, b, r, kinds, 0, o, stream)) return rc;
  if (b->n == 0) return GPK_OK;
  hipStream_t s = (hipStream_t)stream;
  size_t tb = d->tmp2_bytes;
  const CountIn in(hipcub::CountingInputIterator<uint32_t>(0), CountOf{o->records, o->counts});
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp2, tb, in, d->starts, (int)b->n, s) != hipSuccess) return GPK_EHIP;
  const EmitArgs ea{b->data, b->offsets, d->starts, *o};
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((b->n + kBlk - 1) / kBlk)), dim3(kBlk), 0, s, ea);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

extern "C" int gpk_ndp_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                  const gpk_ndps* o) {
  if (bad_out(o, kinds)) return GPK_EINVAL;
  if (const int rc = pass_batch_host<NdpPass>(parser, b, r, kinds, 0, o)) return rc;
  const EmitArgs ea{b->data, b->offsets, nullptr, *o};
  const uint32_t m = o->counts[0];
  uint64_t t = 0;
  for (uint32_t j = 0; j < m; j++) {
    const uint32_t own = o->records[j].nentries;
    emit_one(ea, j, m, t);
    t += own;
  }
  return GPK_OK;
}

extern "C" int gpk_ndp_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  static const char* const kText[] = {
      "ICMP layer less then 4 bytes for ICMPv6 router solicitation",
      "ICMP layer less then 12 bytes for ICMPv6 router advertisement",
      "ICMP layer less then 20 bytes for ICMPv6 neighbor solicitation",
      "ICMP layer less then 20 bytes for ICMPv6 neighbor advertisement",
      "ICMP layer less then 36 bytes for ICMPv6 redirect",
      "ICMP layer less then 2 bytes for ICMPv6 message option",
      "ICMPv6 message option with length 0",
      "ICMP layer only %u bytes for ICMPv6 message option with length %u",
      "ICMP layer less than 20 bytes for Multicast Listener Query Message V1",
      "ICMP layer less than 24 bytes for Multicast Listener Query Message V2",
      "ICMP layer less than %u bytes for Multicast Listener Query Message V2",
      "ICMP layer less than 4 bytes for Multicast Listener Report Message V2",
      "Multicast Listener Report Message V2 layer less than 4 bytes for Multicast Address Record",
      "Multicast Listener Report Message V2 layer less than %u bytes for Multicast Address Record",
      "Multicast Listener Report Message V2 layer less than %u bytes for Multicast Address Record",
  };
  static_assert(sizeof(kText) / sizeof(kText[0]) == GPK_NDP_ERR_END - GPK_NDP_ERR_RS_SHORT, "one text per gpk_ndp_err");
  int n;
  if (err == 0) n = snprintf(buf, cap, "%s", "");
  else if (err < GPK_NDP_ERR_RS_SHORT || err >= GPK_NDP_ERR_END) return GPK_EINVAL;
  else n = snprintf(buf, cap, kText[err - GPK_NDP_ERR_RS_SHORT], a0, a1);  // a text takes none, one or both arguments
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
