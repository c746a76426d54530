// gpk_tunnel.hip — one tunnel level peeled off a decoded batch
// (include/gpk_tunnel.h): the pass of gpk_postpass.h with the
// rules of gpk_tunnel_rules.h. An entry is the gpk_tunnel record and the inner
// slice; the sum is GRE's over Contents‖Payload, for the headers with the C bit.
#include <cstdio>

#include "../../include/gpk_tunnel.h"
#include "gpk_postpass.h"
#include "gpk_tunnel_rules.h"

namespace {

struct TunnelPass {
  using Rec = gpk::tun::Tun;
  using Packed = gpk_tunnel;
  using Out = gpk_tunnels;
  static constexpr int kNC = GPK_TUN_NCLASS, kNone = GPK_TUN_NONE;
  static constexpr uint32_t kAll = GPK_TUN_ALL, kSumFlag = GPK_TUN_GRE_CSUM, kSumGroupBytes = GPK_TUN_SUM_GROUP_BYTES;

  static GPK_HD int decode(const PassArgs<TunnelPass>& a, uint64_t i, Rec& t) {
    return gpk::tun::peel(a.tab, a.kinds, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i], t);
  }
  static GPK_HD bool wants_sum(const Rec& t) { return gpk::tun::wants_sum(t); }
  static GPK_HD void emit(const PassArgs<TunnelPass>& a, uint64_t i, uint32_t pos, Rec& t) {
    if ((a.flags & GPK_TUN_GRE_CSUM) && t.kind == GPK_TUN_GRE && !t.err && !gpk::tun::wants_sum(t))
      t.status |= GPK_TUN_ST_VALID;  // !ChecksumPresent: Valid without a sum (gre.go:246)
    a.out.in_offsets[pos] = a.offsets[i] + t.inner_off;
    a.out.in_caplens[pos] = t.inner_len;
    gpk::tun::tun_store(&a.out.tunnels[pos], t);
  }
  static bool missing(const Out& o) { return !o.in_offsets || !o.in_caplens || !o.tunnels; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.tunnels[j]; }
  static GPK_HD bool entry_wants_sum(const Packed& t) {  // gpk::tun::wants_sum
    return t.kind == GPK_TUN_GRE && !t.err && (t.raw0 & 0x80);
  }
  static GPK_HD uint32_t entry_len(const Packed& t) { return t.contents_len + t.inner_len; }
  static GPK_HD uint32_t start(const SumArgs<TunnelPass>&, const Packed*, uint32_t, uint32_t, uint32_t) { return 0; }
  static GPK_HD void verdict(Packed* t, uint32_t sum, uint32_t) {
    const uint32_t existing = t->gre_checksum, correct = gpk::tun::gre_correct(sum, existing);
    t->gre_correct = (uint16_t)correct;
    t->status = (uint8_t)(t->status | gpk::tun::gre_status(correct, existing));
  }
};

}  // namespace

struct gpk_tunneler : PassHandle<TunnelPass> {};

extern "C" int gpk_tunneler_create(gpk_tunneler** out, int device, uint64_t max_packets) {
  return pass_create(out, device, max_packets, 1ull << 32);
}
extern "C" int gpk_tunneler_destroy(gpk_tunneler* t) { return pass_destroy(t); }
extern "C" int gpk_tunneler_set_sum_threshold(gpk_tunneler* t, uint32_t bytes) {
  return pass_set_sum_threshold(t, bytes);
}
extern "C" int gpk_tunnel_batch(gpk_tunneler* t, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                                const gpk_results* r, uint32_t kinds, uint32_t flags, const gpk_tunnels* o,
                                void* stream) {
  return pass_batch(t, ctx, parser, b, r, kinds, flags, o, stream);
}
extern "C" int gpk_tunnel_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                     uint32_t flags, const gpk_tunnels* o) {
  return pass_batch_host<TunnelPass>(parser, b, r, kinds, flags, o);
}

extern "C" int gpk_tunnel_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  const char* s = nullptr;
  switch (err) {
    case 0: s = ""; break;
    case GPK_TUN_ERR_VXLAN_SMALL: s = "vxlan packet too small"; break;
    case GPK_TUN_ERR_GRE_SMALL: s = "GRE packet too small"; break;
    case GPK_TUN_ERR_GRE_TRUNCATED: s = "GRE packet truncated"; break;
    case GPK_TUN_ERR_GENEVE_OPT_SHORT:
    case GPK_TUN_ERR_GENEVE_OPT_LEN: s = "geneve option too small"; break;
    case GPK_TUN_ERR_GENEVE_SHORT:
    case GPK_TUN_ERR_GENEVE_OPTS_SHORT: s = "geneve packet too short"; break;
    case GPK_ERR_PANIC_INDEX:
    case GPK_ERR_PANIC_SLICE_ACAP:
    case GPK_ERR_PANIC_SLICE_B: return gpk_format_error(err, a0, a1, buf, cap);
    default: return GPK_EINVAL;
  }
  const int n = snprintf(buf, cap, "%s", s);
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
