// gpk_control.hip — the ICMPv4, ICMPv6 (+Echo) and ARP layers at the end of a
// decoded batch (include/gpk_control.h): the pass of
// gpk_postpass.h with the rules of gpk_control_rules.h. An entry is the
// gpk_control record; the sum is ICMPv4's and ICMPv6's over Contents‖Payload.
#include <cstdio>

#include "../../include/gpk_control.h"
#include "gpk_control_rules.h"
#include "gpk_postpass.h"

namespace {

struct ControlPass {
  using Rec = gpk::ctl::Ctl;
  using Packed = gpk_control;
  using Out = gpk_controls;
  static constexpr int kNC = GPK_CTL_NCLASS, kNone = GPK_CTL_NONE;
  static constexpr uint32_t kAll = GPK_CTL_ALL, kSumFlag = GPK_CTL_CSUM, kSumGroupBytes = GPK_CTL_SUM_GROUP_BYTES;

  static GPK_HD int decode(const PassArgs<ControlPass>& a, uint64_t i, Rec& c) {
    return gpk::ctl::control(a.tab, a.kinds, a.flags, a.data + a.offsets[i], a.caplens[i], a.records[i], a.layouts[i],
                             c);
  }
  static GPK_HD bool wants_sum(const Rec& c) { return gpk::ctl::wants_sum(c.kind, c.nlayers, c.status); }
  static GPK_HD void emit(const PassArgs<ControlPass>& a, uint64_t, uint32_t pos, Rec& c) {
    gpk::ctl::ctl_store(&a.out.records[pos], c);
  }
  static bool missing(const Out& o) { return !o.records; }
  static GPK_HD Packed* entry(const Out& o, uint64_t j) { return &o.records[j]; }
  static GPK_HD bool entry_wants_sum(const Packed& r) { return gpk::ctl::wants_sum(r.kind, r.nlayers, r.status); }
  static GPK_HD uint32_t entry_len(const Packed& r) { return r.contents_len + r.payload_len; }
  // An ICMPv6 entry's start value: the pseudo-header's 4 or 16 address words and the
  // length; 0 for ICMPv4. On the device the first 16 lanes of the entry's group (gl <
  // 16) read one word each (one line per group, where a lane of the scatter would
  // touch a line per packet for every word) and reduce them over 16 lanes; every lane
  // of the group returns the value.
  static GPK_HD uint32_t start(const SumArgs<ControlPass>& a, const Packed* r, uint32_t pkt, uint32_t len,
                               uint32_t gl) {
    if (r->kind != GPK_CTL_ICMP6) return 0;
    gpk::ctl::Net net;
    if (!gpk::ctl::network_layer(a.caplens[pkt], a.records[pkt], a.layouts[pkt], net)) return 0;  // not reached: NONET
    const uint8_t* addr = a.data + a.offsets[pkt] + net.off;
    uint32_t w = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    if (2 * gl < net.bytes) w = gpk::ctl::be16(addr + 2 * gl);
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) w += (uint32_t)__shfl_xor((int)w, d, 16);
#else
    for (uint32_t q = 0; q < net.bytes; q += 2) w += gpk::ctl::be16(addr + q);
#endif
    return gpk::ctl::start_value(w, len);
  }
  static GPK_HD void verdict(Packed* r, uint32_t sum, uint32_t start) {
    const uint32_t existing = r->checksum, correct = gpk::ctl::correct_of(sum + start, existing);
    r->sum_init = start;
    r->correct = (uint16_t)correct;
    r->status = (uint8_t)(r->status | gpk::ctl::sum_status(correct, existing));
  }
};

}  // namespace

struct gpk_controller : PassHandle<ControlPass> {};

extern "C" int gpk_controller_create(gpk_controller** out, int device, uint64_t max_packets) {
  return pass_create(out, device, max_packets, 1ull << 28);
}
extern "C" int gpk_controller_destroy(gpk_controller* c) { return pass_destroy(c); }
extern "C" int gpk_controller_set_sum_threshold(gpk_controller* c, uint32_t bytes) {
  return pass_set_sum_threshold(c, bytes);
}
extern "C" int gpk_control_batch(gpk_controller* c, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                                 const gpk_results* r, uint32_t kinds, uint32_t flags, const gpk_controls* o,
                                 void* stream) {
  return pass_batch(c, ctx, parser, b, r, kinds, flags, o, stream);
}
extern "C" int gpk_control_batch_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r, uint32_t kinds,
                                      uint32_t flags, const gpk_controls* o) {
  return pass_batch_host<ControlPass>(parser, b, r, kinds, flags, o);
}

extern "C" int gpk_control_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap) {
  if (!buf || cap == 0) return GPK_EINVAL;
  int n;
  switch (err) {
    case 0: n = snprintf(buf, cap, "%s", ""); break;
    case GPK_CTL_ERR_ICMP4_SHORT: n = snprintf(buf, cap, "ICMP layer less then 8 bytes for ICMPv4 packet"); break;
    case GPK_CTL_ERR_ICMP6_SHORT: n = snprintf(buf, cap, "ICMP layer less then 4 bytes for ICMPv6 packet"); break;
    case GPK_CTL_ERR_ECHO_SHORT: n = snprintf(buf, cap, "ICMP layer less then 4 bytes for ICMPv6 Echo"); break;
    case GPK_CTL_ERR_ARP_SHORT: n = snprintf(buf, cap, "ARP length %u too short", a0); break;
    case GPK_CTL_ERR_ARP_EXPECTED: n = snprintf(buf, cap, "ARP length %u too short, %u expected", a0, a1); break;
    default: return GPK_EINVAL;
  }
  return n < 0 ? GPK_EINVAL : (n >= (int)cap ? (int)cap - 1 : n);
}
