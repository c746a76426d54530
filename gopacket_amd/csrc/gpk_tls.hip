// gpk_tls.hip — the TLS messages at the end of a decoded batch
// (include/gpk_tls.h): the pass of gpk_postpass.h with the rules
// of gpk_tls_rules.h (no sum), then the second stage of gpk_arena.h, which a
// variable-length result needs:
//   scan          exclusive sums of (nrec, nhello, sni_bytes) over the compact
//                 list: where each message's entries and server names start
//   emit_kernel   one lane per message: the walk again, in store mode, when the
//                 message's whole range fits rec_cap, hello_cap and sni_cap
// One lane per message throughout: the record walk is sequential, and the
// common message (one or two Application Data records) is a dozen byte loads
// and one 16-byte entry. The server name bytes are copied by the same lane: a
// name is a few tens of bytes, far below what a cooperative mover needs to pay
// for its dispatch.
#include "../../include/gpk_tls.h"
#include "gpk_arena.h"
#include "gpk_tls_rules.h"

namespace {

struct TlsPass : NoSum {
  using Rec = gpk::tls::Msg;
  using Packed = gpk_tls;
  using Out = gpk_tlss;
  static constexpr int kNC = GPK_TLS_NCLASS, kNone = GPK_TLS_NONE;
  static constexpr uint32_t kAll = GPK_TLS_ALL;

  static GPK_HD int decode(const PassArgs<TlsPass>& a, uint64_t i, Rec& m) {
    return gpk::tls::tls(a.tab, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD void emit(const PassArgs<TlsPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::tls::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }

  static constexpr int kCounts = 12;  // this pass has three totals
  static constexpr uint32_t kDropped = GPK_TLS_ST_DROPPED;
  struct Tot {  // record entries, hello entries and server name bytes in front of a message
    uint64_t rec, hello, sni;
  };
  static GPK_HD Tot own(const Packed& r) { return Tot{r.nrec, r.nhello, r.sni_bytes}; }
  static GPK_HD Tot add(const Tot& a, const Tot& b) { return Tot{a.rec + b.rec, a.hello + b.hello, a.sni + b.sni}; }
  static GPK_HD bool fits(const Out& o, const Tot&, const Tot& end) {
    return end.rec <= o.rec_cap && end.hello <= o.hello_cap && end.sni <= o.sni_cap;
  }
  static GPK_HD void report(uint32_t* c, const Tot& end) {
    put64(c + 4, end.rec), put64(c + 6, end.hello), put64(c + 8, end.sni);
  }
  static GPK_HD void place(Packed* r, const Tot& t) { r->rec0 = t.rec, r->hello0 = t.hello, r->sni0 = t.sni; }
  static GPK_HD void walk(const EmitArgs<TlsPass>& a, uint32_t j, const Packed* r, const Tot& t, const Tot&) {
    const uint32_t pkt = a.out.index[j];
    gpk::tls::Msg msg;
    gpk::tls::msg_init(msg, r->hdr_off);
    gpk::tls::walk<true>(a.data + a.offsets[pkt] + r->hdr_off, r->len, a.caplens[pkt] - r->hdr_off, msg, pkt,
                         a.out.recs + t.rec, a.out.hellos + t.hello, a.out.snis, t.sni);
  }
  static bool bad_out(const Out* o, uint32_t) {
    return !o || ((uintptr_t)o->recs & 7) || ((uintptr_t)o->hellos & 7) || (o->rec_cap && !o->recs) ||
           (o->hello_cap && !o->hellos) || (o->sni_cap && !o->snis);
  }
};

}  // namespace

struct gpk_tls_decoder : ArenaHandle<TlsPass> {
  void carve() { ArenaHandle<TlsPass>::carve(); }  // a member of its own, so the library exports what it did
};

extern "C" int gpk_tls_decoder_create(gpk_tls_decoder** out, int device, uint64_t max_packets) {
  return arena_create(out, device, max_packets);
}
extern "C" int gpk_tls_decoder_destroy(gpk_tls_decoder* d) { return pass_destroy(d); }
extern "C" int gpk_tls_batch(gpk_tls_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, const gpk_tlss* o, void* stream) {
  return arena_batch(d, ctx, parser, b, r, GPK_TLS_ALL, o, stream);
}
extern "C" int gpk_tls_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r,
                                  const gpk_tlss* o) {
  return arena_batch_host<TlsPass>(parser, b, r, GPK_TLS_ALL, o);
}

extern "C" int gpk_tls_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
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
  if (buf && cap && err == GPK_ERR_PANIC_SLICE_B) return gpk_format_error(err, a0, a1, buf, cap);
  return format_text(kText, GPK_TLS_ERR_RECORD_SHORT, GPK_TLS_ERR_END, err, a0, a1, buf, cap);
}
