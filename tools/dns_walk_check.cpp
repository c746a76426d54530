// dns_walk_check.cpp — the DNS walk of csrc/gpk_dns_rules.h (walk<false>, then walk<true>) over a file of
// messages (each: a little-endian 32-bit length, then the bytes), every message, entry and name buffer
// heap-allocated at its exact size, for a run under ASan / UBSan: host code only, no GPU is touched.
// tools/dns_walk_check.py writes the file, builds this and runs it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gpk_dns_rules.h"
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned long msgs = 0, ok = 0, rrs_total = 0, nb_total = 0;
  uint32_t len;
  while (fread(&len, 4, 1, f) == 1) {
    uint8_t* d = (uint8_t*)malloc(len);
    if (fread(d, 1, len, f) != len) return 3;
    gpk::dns::Msg m;
    gpk::dns::msg_init(m, 0);
    gpk::dns::walk<false>(d, len, m, nullptr, nullptr, 0);
    msgs++;
    if (!m.err) {
      ok++;
      gpk_dns_rr* rrs = (gpk_dns_rr*)malloc(m.nrr ? m.nrr * sizeof(gpk_dns_rr) : 1);
      uint8_t* names = (uint8_t*)malloc(m.name_bytes ? m.name_bytes : 1);
      gpk::dns::Msg e;
      gpk::dns::msg_init(e, 0);
      gpk::dns::walk<true>(d, len, e, rrs, names, 0);
      if (e.err || e.nrr != m.nrr || e.name_bytes != m.name_bytes) { printf("modes differ at message %lu\n", msgs); return 1; }
      rrs_total += m.nrr, nb_total += m.name_bytes;
      free(rrs), free(names);
    }
    free(d);
  }
  printf("%lu messages, %lu decoded, %lu entries, %lu name bytes\n", msgs, ok, rrs_total, nb_total);
  return 0;
}
