// gpk_seam.h — the bytes of two buffers end to end, for the one record or
// message of a stream that straddles the carried tail and the new bytes
// (gpk_tls_streams.hip, gpk_dns_streams.hip). The rules that read bytes take
// them as B: a const uint8_t*, or a Seam.
#pragma once
#include <stdint.h>

#include "gpk_tunnel_rules.h"

namespace gpk {

// A logical buffer a[0..na) followed by b[0..): what a const uint8_t* offers the
// rules (index, + offset), over the seam between a stream's tail and its new bytes.
struct Seam {
  const uint8_t* a;
  const uint8_t* b;
  uint32_t na, at;
  GPK_HD uint8_t operator[](uint32_t i) const {
    const uint32_t k = at + i;
    return k < na ? a[k] : b[k - na];
  }
  GPK_HD Seam operator+(uint32_t k) const { return Seam{a, b, na, at + k}; }
};

GPK_HD uint32_t be16(const Seam& p) { return (uint32_t)p[0] << 8 | p[1]; }
GPK_HD uint32_t be32(const Seam& p) { return be16(p) << 16 | be16(p + 2); }

}  // namespace gpk
