// gpk_tls.hip — the TLS messages at the end of a decoded batch
// (include/gpk_tls.h): the pass of gpk_postpass.h with the rules
// of gpk_tls_rules.h (no sum), then what a variable-length result needs:
//   scan          exclusive sums of (nrec, nhello, sni_bytes) over the compact
//                 list: where each message's entries and server names start
//   emit_kernel   one lane per message: the walk again, in store mode, when the
//                 message's whole range fits rec_cap, hello_cap and sni_cap
// One lane per message throughout: the record walk is sequential, and the
// common message (one or two Application Data records) is a dozen byte loads
// and one 16-byte entry. The server name bytes are copied by the same lane: a
// name is a few tens of bytes, far below what a cooperative mover needs to pay
// for its dispatch.
#include <cstdio>

#include "../../include/gpk_tls.h"
#include "gpk_postpass.h"
#include "gpk_tls_rules.h"

namespace {

struct TlsPass {
  using Rec = gpk::tls::Msg;
  using Packed = gpk_tls;
  using Out = gpk_tlss;
  static constexpr int kNC = GPK_TLS_NCLASS, kNone = GPK_TLS_NONE;
  static constexpr uint32_t kAll = GPK_TLS_ALL, kSumFlag = 0, kSumGroupBytes = 0;  // no sum: those kernels never launch

  static GPK_HD int decode(const PassArgs<TlsPass>& a, uint64_t i, Rec& m) {
    return gpk::tls::tls(a.tab, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD bool wants_sum(const Rec&) { return false; }
  static GPK_HD void emit(const PassArgs<TlsPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::tls::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }
  static GPK_HD bool entry_wants_sum(const Packed&) { return false; }
  static GPK_HD uint32_t entry_len(const Packed&) { return 0; }
  static GPK_HD uint32_t start(const SumArgs<TlsPass>&, const Packed*, uint32_t, uint32_t, uint32_t) { return 0; }
  static GPK_HD void verdict(Packed*, uint32_t, uint32_t) {}
};

// record entries, hello entries and server name bytes in front of a message
struct Tot {
  uint64_t rec, hello, sni;
};
struct TotAdd {
  __host__ __device__ Tot operator()(const Tot& a, const Tot& b) const {
    return Tot{a.rec + b.rec, a.hello + b.hello, a.sni + b.sni};
  }
};
struct TotOf {  // of entry j; nothing past m
  const gpk_tls* records;
  const uint32_t* counts;
  __host__ __device__ Tot operator()(uint32_t j) const {
    if (j >= counts[0]) return Tot{0, 0, 0};
    return Tot{records[j].nrec, records[j].nhello, records[j].sni_bytes};
  }
};
using TotIn = hipcub::TransformInputIterator<Tot, TotOf, hipcub::CountingInputIterator<uint32_t>>;

struct EmitArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const Tot* starts;
  gpk_tlss out;
};

GPK_HD bool fits(const gpk_tlss& o, const Tot& t) {
  return t.rec <= o.rec_cap && t.hello <= o.hello_cap && t.sni <= o.sni_cap;
}

// Entry j (< m) of the compact list, t: the totals in front of it. The last
// entry also reports what the batch needs.
GPK_HD void emit_one(const EmitArgs& a, uint32_t j, uint32_t m, const Tot& t) {
  gpk_tls* r = &a.out.records[j];
  const Tot end{t.rec + r->nrec, t.hello + r->nhello, t.sni + r->sni_bytes};
  if (j == m - 1) {
    uint32_t* c = a.out.counts;
    c[3] = !fits(a.out, end);
    c[4] = (uint32_t)end.rec, c[5] = (uint32_t)(end.rec >> 32);
    c[6] = (uint32_t)end.hello, c[7] = (uint32_t)(end.hello >> 32);
    c[8] = (uint32_t)end.sni, c[9] = (uint32_t)(end.sni >> 32);
  }
  if (r->err) return;
  r->rec0 = t.rec;
  r->hello0 = t.hello;
  r->sni0 = t.sni;
  if (!fits(a.out, end)) {
    r->status |= GPK_TLS_ST_DROPPED;
    return;
  }
  const uint32_t pkt = a.out.index[j];
  gpk::tls::Msg msg;
  gpk::tls::msg_init(msg, r->hdr_off);
  gpk::tls::walk<true>(a.data + a.offsets[pkt] + r->hdr_off, r->len, a.caplens[pkt] - r->hdr_off, msg, pkt,
                       a.out.recs + t.rec, a.out.hellos + t.hello, a.out.snis, t.sni);
}

__global__ void __launch_bounds__(kBlk) emit_kernel(const EmitArgs a) {
  const uint32_t m = a.out.counts[0];
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < m) emit_one(a, (uint32_t)j, m, a.starts[j]);
}

bool bad_arena(const gpk_tlss* o) {
  return !o || ((uintptr_t)o->recs & 7) || ((uintptr_t)o->hellos & 7) || (o->rec_cap && !o->recs) ||
         (o->hello_cap && !o->hellos) || (o->sni_cap && !o->snis);
}

}  // namespace

struct gpk_tls_decoder : PassHandle<TlsPass> {
  Tot* starts = nullptr;  // [cap]
  uint8_t* tmp2 = nullptr;
  size_t tmp2_bytes = 0;
  void carve() {
    PassHandle<TlsPass>::carve();
    if (!tmp2_bytes &&
        hipcub::DeviceScan::ExclusiveScan(nullptr, tmp2_bytes, TotIn(hipcub::CountingInputIterator<uint32_t>(0),
                                                                     TotOf{nullptr, nullptr}),
                                          (Tot*)nullptr, TotAdd(), Tot{0, 0, 0}, (int)cap) != hipSuccess)
      tmp2_bytes = 0;
    ws.take(starts, cap);
    ws.take(tmp2, tmp2_bytes ? tmp2_bytes : 4);
  }
};

extern "C" int gpk_tls_decoder_create(gpk_tls_decoder** out, int device, uint64_t max_packets) {
  if (const int rc = pass_create(out, device, max_packets, 1ull << 28)) return rc;
  if ((*out)->tmp2_bytes == 0) {  // the second scan's size query failed in carve(): as pass_create reports the first
    pass_destroy(*out);
    *out = nullptr;
    return GPK_ENOMEM;
  }
  return GPK_OK;
}
extern "C" int gpk_tls_decoder_destroy(gpk_tls_decoder* d) { return pass_destroy(d); }

extern "C" int gpk_tls_batch(gpk_tls_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, const gpk_tlss* o, void* stream) {
  if (!d || bad_arena(o)) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  hipStream_t s = (hipStream_t)stream;
  if (!ctx || bad_args<TlsPass>(parser, b, r, GPK_TLS_ALL, 0, o)) return GPK_EINVAL;
  if (hipMemsetAsync(o->counts + 8, 0, 4 * 4, s) != hipSuccess) return GPK_EHIP;  // the pass zeroes the first eight
  if (const int rc = pass_batch(d, ctx, parser, b, r, GPK_TLS_ALL, 0, o, stream)) return rc;
  if (b->n == 0) return GPK_OK;
  size_t tb = d->tmp2_bytes;
  const TotIn in(hipcub::CountingInputIterator<uint32_t>(0), TotOf{o->records, o->counts});
  if (hipcub::DeviceScan::ExclusiveScan(d->tmp2, tb, in, d->starts, TotAdd(), Tot{0, 0, 0}, (int)b->n, s) !=
      hipSuccess)
    return GPK_EHIP;
  const EmitArgs ea{b->data, b->offsets, b->caplens, d->starts, *o};
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((b->n + kBlk - 1) / kBlk)), dim3(kBlk), 0, s, ea);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

extern "C" int gpk_tls_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r,
                                  const gpk_tlss* o) {
  if (bad_arena(o)) return GPK_EINVAL;
  if (const int rc = pass_batch_host<TlsPass>(parser, b, r, GPK_TLS_ALL, 0, o)) return rc;
  for (int k = 8; k < 12; k++) o->counts[k] = 0;
  const EmitArgs ea{b->data, b->offsets, b->caplens, nullptr, *o};
  const uint32_t m = o->counts[0];
  Tot t{0, 0, 0};
  for (uint32_t j = 0; j < m; j++) {
    const Tot own{o->records[j].nrec, o->records[j].nhello, o->records[j].sni_bytes};
    emit_one(ea, j, m, t);
    t = TotAdd()(t, own);
  }
  return GPK_OK;
}

extern "C" int gpk_tls_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  static const char* const kText[] = {
      "TLS record too short",
      "Unknown TLS record type",
      "TLS packet length mismatch",
      "TLS Change Cipher Spec record incorrect length",
      "TLS Alert packet too short",
      "TLS handshake record too short",
      "Unknown TLS handshake type",
      "TLS ClientHello too short",
      "TLS ClientHello truncated in session ID",
      "TLS ClientHello truncated in cipher suites",
      "TLS ClientHello truncated in compression methods",
      "TLS ClientHello truncated in extensions",
  };
  static_assert(sizeof(kText) / sizeof(kText[0]) == GPK_TLS_ERR_END - GPK_TLS_ERR_RECORD_SHORT,
                "one text per gpk_tls_err");
  int n;
  if (err == 0) n = snprintf(buf, cap, "%s", "");
  else if (err == GPK_ERR_PANIC_SLICE_B) return gpk_format_error(err, a0, a1, buf, cap);
  else if (err < GPK_TLS_ERR_RECORD_SHORT || err >= GPK_TLS_ERR_END) return GPK_EINVAL;
  else n = snprintf(buf, cap, "%s", kText[err - GPK_TLS_ERR_RECORD_SHORT]);
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
