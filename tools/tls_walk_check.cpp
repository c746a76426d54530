// tls_walk_check.cpp — the TLS walk of csrc/gpk_tls_rules.h (walk<false>, then walk<true>) over a file of
// messages (each: little-endian 32-bit message length and buffer length, then the buffer: the message and
// what the packet holds behind it), every buffer, entry and name array heap-allocated at its exact size, for
// a run under ASan / UBSan: host code only, no GPU is touched. tools/tls_walk_check.py writes the file,
// builds this and runs it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "gpk_tls_rules.h"
int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) return 2;
  unsigned long msgs = 0, ok = 0, recs_total = 0, hellos_total = 0, sni_total = 0;
  uint32_t head[2];
  while (fread(head, 4, 2, f) == 2) {
    const uint32_t len = head[0], avail = head[1];
    if (len > avail) return 3;
    uint8_t* d = (uint8_t*)malloc(avail ? avail : 1);
    if (fread(d, 1, avail, f) != avail) return 3;
    gpk::tls::Msg m;
    gpk::tls::msg_init(m, 7);
    gpk::tls::walk<false>(d, len, avail, m, 0, nullptr, nullptr, nullptr, 0);
    msgs++;
    if (!m.err) {
      ok++;
      const uint32_t nrec = m.nccs + m.nalert + m.nhs + m.napp;
      gpk_tls_rec* recs = (gpk_tls_rec*)malloc(nrec ? nrec * sizeof(gpk_tls_rec) : 1);
      gpk_tls_hello* hellos = (gpk_tls_hello*)malloc(m.nhello ? m.nhello * sizeof(gpk_tls_hello) : 1);
      uint8_t* snis = (uint8_t*)malloc(m.sni_bytes ? m.sni_bytes : 1);
      gpk::tls::Msg e;
      gpk::tls::msg_init(e, 7);
      gpk::tls::walk<true>(d, len, avail, e, (uint32_t)msgs, recs, hellos, snis, 0);
      if (e.err || e.nccs != m.nccs || e.nalert != m.nalert || e.nhs != m.nhs || e.napp != m.napp ||
          e.nhello != m.nhello || e.sni_bytes != m.sni_bytes) {
        printf("modes differ at message %lu\n", msgs);
        return 1;
      }
      uint64_t names = 0;  // the hello entries account for every name byte, in order
      for (uint32_t k = 0; k < m.nhello; k++) {
        if (hellos[k].sni_pos != names || hellos[k].packet != (uint32_t)msgs) {
          printf("hello %u of message %lu is out of place\n", k, msgs);
          return 1;
        }
        if (hellos[k].sni_len && memcmp(snis + names, d + (hellos[k].sni_off - 7), hellos[k].sni_len)) {
          printf("name %u of message %lu differs from the packet's bytes\n", k, msgs);
          return 1;
        }
        names += hellos[k].sni_len;
      }
      if (names != m.sni_bytes) return 1;
      recs_total += nrec, hellos_total += m.nhello, sni_total += m.sni_bytes;
      free(recs), free(hellos), free(snis);
    }
    free(d);
  }
  printf("%lu messages, %lu decoded, %lu records, %lu hellos, %lu name bytes\n", msgs, ok, recs_total, hellos_total,
         sni_total);
  return 0;
}
