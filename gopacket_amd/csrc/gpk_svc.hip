// gpk_svc.hip — the DHCPv4, DHCPv6 and NTP messages at the end of a decoded
// batch (include/gpk_svc.h): the pass of gpk_postpass.h with the
// rules of gpk_svc_rules.h (no sum), then what a variable-length result needs:
//   scan          exclusive sums of nentries over the compact list: where each
//                 message's entries start
//   emit_kernel   one lane per message: stores entry0 and, when the message's
//                 whole range fits entry_cap, walks again in emit form
#include <cstdio>

#include "../../include/gpk_svc.h"
#include "gpk_svc_rules.h"
#include "gpk_postpass.h"

namespace {

struct SvcPass {
  using Rec = gpk::svc::Msg;
  using Packed = gpk_svc;
  using Out = gpk_svcs;
  static constexpr int kNC = GPK_SVC_NCLASS, kNone = GPK_SVC_NONE;
  static constexpr uint32_t kAll = GPK_SVC_ALL, kSumFlag = 0, kSumGroupBytes = 0;  // no sum: those kernels never launch

  static GPK_HD int decode(const PassArgs<SvcPass>& a, uint64_t i, Rec& m) {
    return gpk::svc::svc(a.tab, a.kinds, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD bool wants_sum(const Rec&) { return false; }
  static GPK_HD void emit(const PassArgs<SvcPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::svc::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }
  static GPK_HD bool entry_wants_sum(const Packed&) { return false; }
  static GPK_HD uint32_t entry_len(const Packed&) { return 0; }
  static GPK_HD uint32_t start(const SumArgs<SvcPass>&, const Packed*, uint32_t, uint32_t, uint32_t) { return 0; }
  static GPK_HD void verdict(Packed*, uint32_t, uint32_t) {}
};

struct CountOf {  // entries of message j; nothing past m
  const gpk_svc* records;
  const uint32_t* counts;
  __host__ __device__ uint64_t operator()(uint32_t j) const { return j < counts[0] ? records[j].nentries : 0; }
};
using CountIn = hipcub::TransformInputIterator<uint64_t, CountOf, hipcub::CountingInputIterator<uint32_t>>;

struct EmitArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint64_t* starts;
  gpk_svcs out;
};

// Entry j (< m) of the compact list, t: the entries in front of it. The last
// one also reports what the batch needs.
GPK_HD void emit_one(const EmitArgs& a, uint32_t j, uint32_t m, uint64_t t) {
  gpk_svc* r = &a.out.records[j];
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
    r->status |= GPK_SVC_ST_DROPPED;
    return;
  }
  gpk::svc::Msg msg;
  gpk::svc::msg_init(msg, r->layer_type, r->hdr_off);
  gpk::svc::walk<true>(a.data + a.offsets[a.out.index[j]] + r->hdr_off, r->len, msg, a.out.entries + t);
}

__global__ void __launch_bounds__(kBlk) emit_kernel(const EmitArgs a) {
  const uint32_t m = a.out.counts[0];
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < m) emit_one(a, (uint32_t)j, m, a.starts[j]);
}

bool bad_out(const gpk_svcs* o) { return !o || ((uintptr_t)o->entries & 7) || (o->entry_cap && !o->entries); }

}  // namespace

struct gpk_svc_decoder : PassHandle<SvcPass> {
  uint64_t* starts = nullptr;  // [cap]
  uint8_t* tmp2 = nullptr;
  size_t tmp2_bytes = 0;
  void carve() {
    PassHandle<SvcPass>::carve();
    if (!tmp2_bytes &&
        hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2_bytes,
                                         CountIn(hipcub::CountingInputIterator<uint32_t>(0), CountOf{nullptr, nullptr}),
                                         (uint64_t*)nullptr, (int)cap) != hipSuccess)
      tmp2_bytes = 0;
    ws.take(starts, cap);
    ws.take(tmp2, tmp2_bytes ? tmp2_bytes : 4);
  }
};

extern "C" int gpk_svc_decoder_create(gpk_svc_decoder** out, int device, uint64_t max_packets) {
  if (const int rc = pass_create(out, device, max_packets, 1ull << 28)) return rc;
  if ((*out)->tmp2_bytes == 0) {  // the second scan's size query failed in carve(): as pass_create reports the first
    pass_destroy(*out);
    *out = nullptr;
    return GPK_ENOMEM;
  }
  return GPK_OK;
}
extern "C" int gpk_svc_decoder_destroy(gpk_svc_decoder* d) { return pass_destroy(d); }

extern "C" int gpk_svc_batch(gpk_svc_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, uint32_t kinds, const gpk_svcs* o, void* stream) {
  if (!d || bad_out(o)) return GPK_EINVAL;
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

extern "C" int gpk_svc_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                  const gpk_svcs* o) {
  if (bad_out(o)) return GPK_EINVAL;
  if (const int rc = pass_batch_host<SvcPass>(parser, b, r, kinds, 0, o)) return rc;
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

extern "C" int gpk_svc_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  static const char* const kText[] = {
      "DHCPv4 length %u too short",
      "DHCPv4 hardware address length %u exceeds 16",
      "Bad DHCP header",
      "Not enough data to decode",
      "Option is malformed",
      "DHCPv6 length %u too short",
      "DHCPv6 length %u too short for message type %u",
      "not enough data to decode",
      "dhcpv6 option size < length %u",
      "NTP packet too short",
  };
  static_assert(sizeof(kText) / sizeof(kText[0]) == GPK_SVC_ERR_END - GPK_SVC_ERR_DHCP4_SHORT, "one text per gpk_svc_err");
  int n;
  if (err == 0) n = snprintf(buf, cap, "%s", "");
  else if (err == GPK_ERR_PANIC_SLICE_B) return gpk_format_error(err, a0, a1, buf, cap);
  else if (err < GPK_SVC_ERR_DHCP4_SHORT || err >= GPK_SVC_ERR_END) return GPK_EINVAL;
  else n = snprintf(buf, cap, kText[err - GPK_SVC_ERR_DHCP4_SHORT], a0, a1);  // a text takes none, one or both arguments
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
