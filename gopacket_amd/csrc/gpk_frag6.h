// gpk_frag6.h — where a packet's IPv6 Fragment header is, for ip6defrag
// (include/gpk_defrag6.h, harness rules): the grouping key (gpk_flows.hip,
// GPK_GROUP_DEFRAG6) and the reassembly's prep kernel (gpk_defrag6.hip) walk
// the same way, so a packet that is keyed always has the fields prep reads.
#ifndef GPK_FRAG6_H
#define GPK_FRAG6_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gpk {

struct Frag6 {
  uint32_t hdr;  // the 8-byte Fragment header, relative to the IPv6 header's start
  uint32_t end;  // end of the IPv6 payload as DecodeFromBytes trimmed it, same base
};

// ip[0..len) is the range a successful IPv6.DecodeFromBytes was given (the
// layout slot). The walk starts at the LayerPayload() and next header that
// decode left (ip6.go:235-275: an inline HopByHop consumed, except for a
// jumbogram, whose payload starts at the HopByHop header; trimmed to Length or
// the jumbo length), skips headers 0, 43 and 60 as decodeIPv6ExtensionBase
// reads them (ip6.go:418-432) and ends at the first next-header 44 with 8
// bytes there. Anything else: not a fragment.
__device__ __forceinline__ bool find_frag6(const uint8_t* ip, uint32_t len, Frag6* out) {
  if (len < 40) return false;
  const uint32_t length = (uint32_t)ip[4] << 8 | ip[5];
  uint32_t nh = ip[6], poff = 40, plen = len - 40, pend = length;
  if (nh == 0) {  // IPv6HopByHop, decoded inline
    if (plen < 8) return false;
    const uint32_t actual = ((uint32_t)ip[41] + 1) * 8;
    if (plen < actual) return false;
    nh = ip[40];
    if (length == 0) {  // a jumbogram (the decode succeeded): the first Jumbo TLV's length
      pend = 0;
      for (uint32_t o = 2; o < actual && o + 1 < plen;) {  // ip6.go:516-524: TLVs are checked against the payload
        const uint32_t t = ip[40 + o];
        if (t == 0) {
          o += 1;
          continue;
        }
        if (t == 0xC2) {
          if (o + 6 <= plen)
            pend = (uint32_t)ip[42 + o] << 24 | (uint32_t)ip[43 + o] << 16 | (uint32_t)ip[44 + o] << 8 | ip[45 + o];
          break;
        }
        o += (uint32_t)ip[41 + o] + 2;
      }
    } else {
      poff += actual;
      plen -= actual;
    }
  }
  if (pend > plen) pend = plen;
  const uint32_t end = poff + pend;
  for (;;) {
    const uint32_t rem = end - poff;
    if (nh == 44) {
      if (rem < 8) return false;
      out->hdr = poff;
      out->end = end;
      return true;
    }
    if (nh != 0 && nh != 43 && nh != 60) return false;
    if (rem < 2) return false;
    const uint32_t actual = ((uint32_t)ip[poff + 1] + 1) * 8;
    if (rem < actual) return false;
    nh = ip[poff];
    poff += actual;
  }
}

}  // namespace gpk
#endif  // GPK_FRAG6_H
