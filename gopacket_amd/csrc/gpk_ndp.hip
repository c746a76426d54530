// gpk_ndp.hip — the NDP and MLD messages behind ICMPv6 at the end of a decoded
// batch (include/gpk_ndp.h): the pass of gpk_postpass.h with the
// rules of gpk_ndp_rules.h (no sum), then the second stage of gpk_arena.h,
// which a variable-length result needs:
//   scan          exclusive sums of nentries over the compact list: where each
//                 message's entries start
//   emit_kernel   one lane per message: stores entry0 and, when the message's
//                 whole range fits entry_cap, walks again in emit form
#include "../../include/gpk_ndp.h"
#include "gpk_ndp_rules.h"
#include "gpk_arena.h"

namespace {

struct NdpPass : NoSum {
  using Rec = gpk::ndp::Msg;
  using Packed = gpk_ndp;
  using Out = gpk_ndps;
  static constexpr int kNC = GPK_NDP_NCLASS, kNone = GPK_NDP_NONE;
  static constexpr uint32_t kAll = GPK_NDP_ALL;

  static GPK_HD int decode(const PassArgs<NdpPass>& a, uint64_t i, Rec& m) {
    return gpk::ndp::ndp(a.tab, a.kinds, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD void emit(const PassArgs<NdpPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::ndp::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }

  static constexpr int kCounts = 8;
  static constexpr uint32_t kDropped = GPK_NDP_ST_DROPPED;
  using Tot = uint64_t;  // entries in front of a message
  static GPK_HD Tot own(const Packed& r) { return r.nentries; }
  static GPK_HD Tot add(Tot a, Tot b) { return a + b; }
  // a message without entries is never dropped: it stores nothing
  static GPK_HD bool fits(const Out& o, Tot t, Tot end) { return end == t || end <= o.entry_cap; }
  static GPK_HD void report(uint32_t* c, Tot end) { put64(c + 4, end); }
  static GPK_HD void place(Packed* r, Tot t) { r->entry0 = t; }
  static GPK_HD void walk(const EmitArgs<NdpPass>& a, uint32_t j, const Packed* r, Tot t, Tot end) {
    if (end == t) return;
    gpk::ndp::Msg msg;
    gpk::ndp::msg_init(msg, r->layer_type, r->hdr_off);
    gpk::ndp::walk<true>(a.data + a.offsets[a.out.index[j]] + r->hdr_off, r->len, msg, a.out.entries + t);
  }
  static bool bad_out(const Out* o, uint32_t kinds) {
    return !o || ((uintptr_t)o->entries & 7) || (o->entry_cap && !o->entries) || kinds == GPK_NDP_ICMP6;
  }
};

}  // namespace

struct gpk_ndp_decoder : ArenaHandle<NdpPass> {
  void carve() { ArenaHandle<NdpPass>::carve(); }  // a member of its own, so the library exports what it did
};

extern "C" int gpk_ndp_decoder_create(gpk_ndp_decoder** out, int device, uint64_t max_packets) {
  return arena_create(out, device, max_packets);
}
extern "C" int gpk_ndp_decoder_destroy(gpk_ndp_decoder* d) { return pass_destroy(d); }
extern "C" int gpk_ndp_batch(gpk_ndp_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, uint32_t kinds, const gpk_ndps* o, void* stream) {
  return arena_batch(d, ctx, parser, b, r, kinds, o, stream);
}
extern "C" int gpk_ndp_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                  const gpk_ndps* o) {
  return arena_batch_host<NdpPass>(parser, b, r, kinds, o);
}

extern "C" int gpk_ndp_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
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
  return format_text(kText, GPK_NDP_ERR_RS_SHORT, GPK_NDP_ERR_END, err, a0, a1, buf, cap);
}
