// gpk_dns.hip — the DNS messages at the end of a decoded batch
// (include/gpk_dns.h): the pass of gpk_postpass.h with the rules
// of gpk_dns_rules.h (no sum), then what a variable-length result needs:
//   scan          exclusive sums of (nrr, name_bytes) over the compact list:
//                 where each message's entries and names start
//   emit_kernel   one lane per message: the walk again, in emit mode, when the
//                 message's whole range fits rr_cap and name_cap
#include <cstdio>

#include "../../include/gpk_dns.h"
#include "gpk_dns_rules.h"
#include "gpk_postpass.h"

namespace {

struct DnsPass {
  using Rec = gpk::dns::Msg;
  using Packed = gpk_dns;
  using Out = gpk_dnss;
  static constexpr int kNC = GPK_DNS_NCLASS, kNone = GPK_DNS_NONE;
  static constexpr uint32_t kAll = GPK_DNS_ALL, kSumFlag = 0, kSumGroupBytes = 0;  // no sum: those kernels never launch

  static GPK_HD int decode(const PassArgs<DnsPass>& a, uint64_t i, Rec& m) {
    return gpk::dns::dns(a.tab, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD bool wants_sum(const Rec&) { return false; }
  static GPK_HD void emit(const PassArgs<DnsPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::dns::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }
  static GPK_HD bool entry_wants_sum(const Packed&) { return false; }
  static GPK_HD uint32_t entry_len(const Packed&) { return 0; }
  static GPK_HD uint32_t start(const SumArgs<DnsPass>&, const Packed*, uint32_t, uint32_t, uint32_t) { return 0; }
  static GPK_HD void verdict(Packed*, uint32_t, uint32_t) {}
};

// entries and name bytes in front of a message
struct Tot {
  uint64_t rr, nb;
};
struct TotAdd {
  __host__ __device__ Tot operator()(const Tot& a, const Tot& b) const { return Tot{a.rr + b.rr, a.nb + b.nb}; }
};
struct TotOf {  // of entry j; nothing past m
  const gpk_dns* records;
  const uint32_t* counts;
  __host__ __device__ Tot operator()(uint32_t j) const {
    if (j >= counts[0]) return Tot{0, 0};
    return Tot{records[j].nrr, records[j].name_bytes};
  }
};
using TotIn = hipcub::TransformInputIterator<Tot, TotOf, hipcub::CountingInputIterator<uint32_t>>;

struct EmitArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const Tot* starts;
  gpk_dnss out;
};

// Entry j (< m) of the compact list, t: the totals in front of it. The last
// entry also reports what the batch needs.
GPK_HD void emit_one(const EmitArgs& a, uint32_t j, uint32_t m, const Tot& t) {
  gpk_dns* r = &a.out.records[j];
  if (j == m - 1) {
    const uint64_t rr = t.rr + r->nrr, nb = t.nb + r->name_bytes;
    a.out.counts[3] = rr > a.out.rr_cap || nb > a.out.name_cap;
    a.out.counts[4] = (uint32_t)rr, a.out.counts[5] = (uint32_t)(rr >> 32);
    a.out.counts[6] = (uint32_t)nb, a.out.counts[7] = (uint32_t)(nb >> 32);
  }
  if (r->err) return;
  r->rr0 = t.rr;
  r->name0 = t.nb;
  if (t.rr + r->nrr > a.out.rr_cap || t.nb + r->name_bytes > a.out.name_cap) {
    r->status |= GPK_DNS_ST_DROPPED;
    return;
  }
  gpk::dns::Msg msg;
  gpk::dns::msg_init(msg, r->hdr_off);
  gpk::dns::walk<true>(a.data + a.offsets[a.out.index[j]] + r->hdr_off, r->len, msg, a.out.rrs + t.rr, a.out.names,
                       t.nb);
}

__global__ void __launch_bounds__(kBlk) emit_kernel(const EmitArgs a) {
  const uint32_t m = a.out.counts[0];
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < m) emit_one(a, (uint32_t)j, m, a.starts[j]);
}

bool bad_arena(const gpk_dnss* o) {
  return !o || ((uintptr_t)o->rrs & 7) || (o->rr_cap && !o->rrs) || (o->name_cap && !o->names);
}

}  // namespace

struct gpk_dns_decoder : PassHandle<DnsPass> {
  Tot* starts = nullptr;  // [cap]
  uint8_t* tmp2 = nullptr;
  size_t tmp2_bytes = 0;
  void carve() {
    PassHandle<DnsPass>::carve();
    if (!tmp2_bytes &&
        hipcub::DeviceScan::ExclusiveScan(nullptr, tmp2_bytes, TotIn(hipcub::CountingInputIterator<uint32_t>(0),
                                                                     TotOf{nullptr, nullptr}),
                                          (Tot*)nullptr, TotAdd(), Tot{0, 0}, (int)cap) != hipSuccess)
      tmp2_bytes = 0;
    ws.take(starts, cap);
    ws.take(tmp2, tmp2_bytes ? tmp2_bytes : 4);
  }
};

extern "C" int gpk_dns_decoder_create(gpk_dns_decoder** out, int device, uint64_t max_packets) {
  if (const int rc = pass_create(out, device, max_packets, 1ull << 28)) return rc;
  if ((*out)->tmp2_bytes == 0) {  // the second scan's size query failed in carve(): as pass_create reports the first
    pass_destroy(*out);
    *out = nullptr;
    return GPK_ENOMEM;
  }
  return GPK_OK;
}
extern "C" int gpk_dns_decoder_destroy(gpk_dns_decoder* d) { return pass_destroy(d); }

extern "C" int gpk_dns_batch(gpk_dns_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, const gpk_dnss* o, void* stream) {
  if (!d || bad_arena(o)) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (const int rc = pass_batch(d, ctx, parser, b, r, GPK_DNS_ALL, 0, o, stream)) return rc;
  if (b->n == 0) return GPK_OK;
  hipStream_t s = (hipStream_t)stream;
  size_t tb = d->tmp2_bytes;
  const TotIn in(hipcub::CountingInputIterator<uint32_t>(0), TotOf{o->records, o->counts});
  if (hipcub::DeviceScan::ExclusiveScan(d->tmp2, tb, in, d->starts, TotAdd(), Tot{0, 0}, (int)b->n, s) != hipSuccess)
    return GPK_EHIP;
  const EmitArgs ea{b->data, b->offsets, d->starts, *o};
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((b->n + kBlk - 1) / kBlk)), dim3(kBlk), 0, s, ea);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

extern "C" int gpk_dns_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r,
                                  const gpk_dnss* o) {
  if (bad_arena(o)) return GPK_EINVAL;
  if (const int rc = pass_batch_host<DnsPass>(parser, b, r, GPK_DNS_ALL, 0, o)) return rc;
  const EmitArgs ea{b->data, b->offsets, nullptr, *o};
  const uint32_t m = o->counts[0];
  Tot t{0, 0};
  for (uint32_t j = 0; j < m; j++) {
    const Tot own{o->records[j].nrr, o->records[j].name_bytes};
    emit_one(ea, j, m, t);
    t = TotAdd()(t, own);
  }
  return GPK_OK;
}

extern "C" int gpk_dns_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  static const char* const kText[] = {
      "DNS packet too short",
      "max DNS recursion level hit",
      "dns name offset too high",
      "dns name is too long",
      "dns name uncomputable: invalid index",
      "dns offset pointer too high",
      "dns index walked out of range",
      "qname '0x40' - RFC 2673 unsupported yet (data=%x index=%u)",
      "qname '0x80' unsupported yet (data=%x index=%u)",
      "DNS question too small",
      "DNS record too small",
      "resource record length exceeds data",
      "Insufficient data for a <character-string>",
      "SOA too small",
      "MX too small",
      "URI too small",
      "SRV too small",
      "NAPTR too small",
      "NAPTR Flags missing",
      "NAPTR Flags truncated",
      "NAPTR Service missing",
      "NAPTR Service truncated",
      "NAPTR Regexp missing",
      "NAPTR Regexp truncated",
      "DNSOPT record is of length %u, it should be at least length 4",
      "Malformed DNSOPT record.  Length %u < %u",
      "Malformed DNSOPT record. The length (%u) field implies a packet larger than the one received",
      "DNSSVCB record is of length %u, it should be at least length 3",
      "DNSSVCB record truncated in SvcParams",
      "RRSIG too small",
      "DNSKEY too small",
  };
  static_assert(sizeof(kText) / sizeof(kText[0]) == GPK_DNS_ERR_END - GPK_DNS_ERR_SHORT, "one text per gpk_dns_err");
  int n;
  if (err == 0) n = snprintf(buf, cap, "%s", "");
  else if (err < GPK_DNS_ERR_SHORT || err >= GPK_DNS_ERR_END) return GPK_EINVAL;
  else n = snprintf(buf, cap, kText[err - GPK_DNS_ERR_SHORT], a0, a1);  // a text takes none, one or both arguments
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
