// gpk_svc.hip — the DHCPv4, DHCPv6 and NTP messages at the end of a decoded
// batch (include/gpk_svc.h): the pass of gpk_postpass.h with the
// rules of gpk_svc_rules.h (no sum), then the second stage of gpk_arena.h,
// which a variable-length result needs:
//   scan          exclusive sums of nentries over the compact list: where each
//                 message's entries start
//   emit_kernel   one lane per message: stores entry0 and, when the message's
//                 whole range fits entry_cap, walks again in emit form
#include "../../include/gpk_svc.h"
#include "gpk_svc_rules.h"
#include "gpk_arena.h"

namespace {

struct SvcPass : NoSum {
  using Rec = gpk::svc::Msg;
  using Packed = gpk_svc;
  using Out = gpk_svcs;
  static constexpr int kNC = GPK_SVC_NCLASS, kNone = GPK_SVC_NONE;
  static constexpr uint32_t kAll = GPK_SVC_ALL;

  static GPK_HD int decode(const PassArgs<SvcPass>& a, uint64_t i, Rec& m) {
    return gpk::svc::svc(a.tab, a.kinds, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD void emit(const PassArgs<SvcPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::svc::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }

  static constexpr int kCounts = 8;
  static constexpr uint32_t kDropped = GPK_SVC_ST_DROPPED;
  using Tot = uint64_t;  // entries in front of a message
  static GPK_HD Tot own(const Packed& r) { return r.nentries; }
  static GPK_HD Tot add(Tot a, Tot b) { return a + b; }
  // a message without entries is never dropped: it stores nothing
  static GPK_HD bool fits(const Out& o, Tot t, Tot end) { return end == t || end <= o.entry_cap; }
  static GPK_HD void report(uint32_t* c, Tot end) { put64(c + 4, end); }
  static GPK_HD void place(Packed* r, Tot t) { r->entry0 = t; }
  static GPK_HD void walk(const EmitArgs<SvcPass>& a, uint32_t j, const Packed* r, Tot t, Tot end) {
    if (end == t) return;
    gpk::svc::Msg msg;
    gpk::svc::msg_init(msg, r->layer_type, r->hdr_off);
    gpk::svc::walk<true>(a.data + a.offsets[a.out.index[j]] + r->hdr_off, r->len, msg, a.out.entries + t);
  }
  static bool bad_out(const Out* o, uint32_t) {
    return !o || ((uintptr_t)o->entries & 7) || (o->entry_cap && !o->entries);
  }
};

}  // namespace

struct gpk_svc_decoder : ArenaHandle<SvcPass> {
  void carve() { ArenaHandle<SvcPass>::carve(); }  // a member of its own, so the library exports what it did
};

extern "C" int gpk_svc_decoder_create(gpk_svc_decoder** out, int device, uint64_t max_packets) {
  return arena_create(out, device, max_packets);
}
extern "C" int gpk_svc_decoder_destroy(gpk_svc_decoder* d) { return pass_destroy(d); }
extern "C" int gpk_svc_batch(gpk_svc_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, uint32_t kinds, const gpk_svcs* o, void* stream) {
  return arena_batch(d, ctx, parser, b, r, kinds, o, stream);
}
extern "C" int gpk_svc_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                  const gpk_svcs* o) {
  return arena_batch_host<SvcPass>(parser, b, r, kinds, o);
}

extern "C" int gpk_svc_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
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
  if (buf && cap && err == GPK_ERR_PANIC_SLICE_B) return gpk_format_error(err, a0, a1, buf, cap);
  return format_text(kText, GPK_SVC_ERR_DHCP4_SHORT, GPK_SVC_ERR_END, err, a0, a1, buf, cap);
}
