// svc_walk_check.cpp — both forms of the UDP service walk (gopacket_amd/csrc/
// gpk_svc_rules.h) over a file of messages, on the host, for a build with
// -fsanitize=address,undefined (tools/svc_walk_check.py builds and drives it).
// Every message is copied into a heap block of exactly its length and every
// entry buffer is allocated at exactly nentries entries, so a read or a write
// one byte past either is a sanitizer report.
//
//   in:  "SVCW" u32 count, then per message u32 layer type, u32 hdr_off, u32 len, len bytes
//   out: per message the packed gpk_svc of the counting form (64 bytes), then
//        the nentries gpk_svc_entry of the emit form
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gopacket_amd/csrc/gpk_svc_rules.h"

static bool get(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s MESSAGES OUT\n", argv[0]), 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
  char magic[4];
  uint32_t count = 0;
  if (!get(in, magic, 4) || memcmp(magic, "SVCW", 4) || !get(in, &count, 4)) return fprintf(stderr, "bad header\n"), 2;
  uint64_t entries = 0, failed = 0;
  for (uint32_t k = 0; k < count; k++) {
    uint32_t head[3];
    if (!get(in, head, sizeof head)) return fprintf(stderr, "short file at message %u\n", k), 2;
    const uint32_t lt = head[0], hdr_off = head[1], len = head[2];
    uint8_t* d = (uint8_t*)malloc(len ? len : 1);  // exactly len bytes (malloc(0) may return null)
    if (len && !get(in, d, len)) return fprintf(stderr, "short file in message %u\n", k), 2;
    gpk::svc::Msg m;
    gpk::svc::msg_init(m, lt, hdr_off);
    gpk::svc::walk<false>(d, len, m, nullptr);
    gpk_svc rec;
    gpk::svc::msg_store(&rec, m);
    fwrite(&rec, sizeof rec, 1, out);
    failed += m.err != 0;
    if (!m.err && m.nentries) {
      gpk_svc_entry* e = (gpk_svc_entry*)malloc(sizeof(gpk_svc_entry) * m.nentries);
      gpk::svc::Msg again;
      gpk::svc::msg_init(again, lt, hdr_off);
      gpk::svc::walk<true>(d, len, again, e);
      if (again.nentries != m.nentries || again.err) return fprintf(stderr, "the two forms disagree at message %u\n", k), 1;
      fwrite(e, sizeof(gpk_svc_entry), m.nentries, out);
      entries += m.nentries;
      free(e);
    }
    free(d);
  }
  fclose(in);
  fclose(out);
  printf("svc_walk_check ok: %u messages, %llu failed, %llu entries\n", count, (unsigned long long)failed,
         (unsigned long long)entries);
  return 0;
}
