// gpk_dns.hip — the DNS messages at the end of a decoded batch
// (include/gpk_dns.h): the pass of gpk_postpass.h with the rules
// of gpk_dns_rules.h (no sum), then the second stage of gpk_arena.h, which a
// variable-length result needs:
//   scan          exclusive sums of (nrr, name_bytes) over the compact list:
//                 where each message's entries and names start
//   emit_kernel   one lane per message: the walk again, in emit mode, when the
//                 message's whole range fits rr_cap and name_cap
#include "../../include/gpk_dns.h"
#include "gpk_dns_rules.h"
#include "gpk_arena.h"

namespace {

struct DnsPass : NoSum {
  using Rec = gpk::dns::Msg;
  using Packed = gpk_dns;
  using Out = gpk_dnss;
  static constexpr int kNC = GPK_DNS_NCLASS, kNone = GPK_DNS_NONE;
  static constexpr uint32_t kAll = GPK_DNS_ALL;

  static GPK_HD int decode(const PassArgs<DnsPass>& a, uint64_t i, Rec& m) {
    return gpk::dns::dns(a.tab, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], m);
  }
  static GPK_HD void emit(const PassArgs<DnsPass>& a, uint64_t, uint32_t pos, Rec& m) {
    gpk::dns::msg_store(&a.out.records[pos], m);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }

  static constexpr int kCounts = 8;
  static constexpr uint32_t kDropped = GPK_DNS_ST_DROPPED;
  struct Tot {  // entries and name bytes in front of a message
    uint64_t rr, nb;
  };
  static GPK_HD Tot own(const Packed& r) { return Tot{r.nrr, r.name_bytes}; }
  static GPK_HD Tot add(const Tot& a, const Tot& b) { return Tot{a.rr + b.rr, a.nb + b.nb}; }
  static GPK_HD bool fits(const Out& o, const Tot&, const Tot& end) {
    return end.rr <= o.rr_cap && end.nb <= o.name_cap;
  }
  static GPK_HD void report(uint32_t* c, const Tot& end) { put64(c + 4, end.rr), put64(c + 6, end.nb); }
  static GPK_HD void place(Packed* r, const Tot& t) { r->rr0 = t.rr, r->name0 = t.nb; }
  static GPK_HD void walk(const EmitArgs<DnsPass>& a, uint32_t j, const Packed* r, const Tot& t, const Tot&) {
    gpk::dns::Msg msg;
    gpk::dns::msg_init(msg, r->hdr_off);
    gpk::dns::walk<true>(a.data + a.offsets[a.out.index[j]] + r->hdr_off, r->len, msg, a.out.rrs + t.rr, a.out.names,
                         t.nb);
  }
  static bool bad_out(const Out* o, uint32_t) {
    return !o || ((uintptr_t)o->rrs & 7) || (o->rr_cap && !o->rrs) || (o->name_cap && !o->names);
  }
};

}  // namespace

struct gpk_dns_decoder : ArenaHandle<DnsPass> {
  void carve() { ArenaHandle<DnsPass>::carve(); }  // a member of its own, so the library exports what it did
};

extern "C" int gpk_dns_decoder_create(gpk_dns_decoder** out, int device, uint64_t max_packets) {
  return arena_create(out, device, max_packets);
}
extern "C" int gpk_dns_decoder_destroy(gpk_dns_decoder* d) { return pass_destroy(d); }
extern "C" int gpk_dns_batch(gpk_dns_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                             const gpk_results* r, const gpk_dnss* o, void* stream) {
  return arena_batch(d, ctx, parser, b, r, GPK_DNS_ALL, o, stream);
}
extern "C" int gpk_dns_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r,
                                  const gpk_dnss* o) {
  return arena_batch_host<DnsPass>(parser, b, r, GPK_DNS_ALL, o);
}

extern "C" int gpk_dns_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
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
  return format_text(kText, GPK_DNS_ERR_SHORT, GPK_DNS_ERR_END, err, a0, a1, buf, cap);
}
