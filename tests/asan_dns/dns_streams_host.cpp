// dns_streams_host.cpp — gpk_dns_streams_host under AddressSanitizer + UBSan: a
// stand-alone driver over a corpus file of recorded calls (written by
// tests/test_dns_streams_asan_cpu.py from dnsstreamcases.py and the model). Every
// array of a call lives in a heap block of exactly its size, so a read or
// write past any of them is reported; the outputs are compared with the
// model's, byte for byte.
//
// Corpus: "DNSS" u32 ncalls, then per call a sequence of blocks, each u64
// length + bytes, in the order of the enum below, the scalars as one block of u64.
//
// The two entries of gpk_host.cpp that the source uses are supplied here: the
// parser's tables (TCP ports 53 and 8080 lead to LayerTypeDNS, as the cases'
// parser has them) and the device-table step, which a host run never takes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpk_device.h"
#include "../../include/gpk_dns_streams.h"

static gpk::DevTables* g_tables;

extern "C" const gpk::DevTables* gpk_parser_tables(const gpk_parser*) { return g_tables; }
extern "C" int gpk_with_device_tables(gpk_ctx*, const gpk_parser*, void*, int (*)(const gpk::DevTables*, void*),
                                      void*) {
  return GPK_EHIP;
}

struct Block {
  uint8_t* p = nullptr;
  uint64_t n = 0;
  ~Block() { free(p); }
};

static bool read_block(FILE* f, Block& b) {
  if (fread(&b.n, 8, 1, f) != 1) return false;
  b.p = (uint8_t*)malloc(b.n ? b.n : 1);
  return b.p && (b.n == 0 || fread(b.p, 1, b.n, f) == b.n);
}

enum { kScalars, kData, kOffsets, kCaplens, kRecords, kLayouts, kChunks, kFirst, kClosed, kData0, kAsmCounts, kAsmData,
       kInState, kInOff, kInLen, kInTails, kStreams, kMsgs, kRrs, kNames, kTails, kCounts, kBlocks };

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  g_tables = new gpk::DevTables();
  for (int i = 0; i < 65536; i++) g_tables->tcp_port[i] = GPK_LT_PAYLOAD;
  g_tables->tcp_port[53] = g_tables->tcp_port[8080] = GPK_LT_DNS;
  char magic[4];
  uint32_t ncalls = 0;
  if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "DNSS", 4) || fread(&ncalls, 4, 1, f) != 1) return 2;
  int bad = 0;
  for (uint32_t c = 0; c < ncalls; c++) {
    Block b[kBlocks];
    for (int k = 0; k < kBlocks; k++)
      if (!read_block(f, b[k])) return 2;
    // scalars: n, chunk_cap, data_cap, nin, flags, fill, max_msg_len
    const uint64_t* s = (const uint64_t*)b[kScalars].p;
    const uint64_t n = s[0], fill = s[5];
    gpk_batch batch{b[kData].p, (const uint64_t*)b[kOffsets].p, (const uint32_t*)b[kCaplens].p, n, b[kData].n};
    gpk_results res{(gpk_record*)b[kRecords].p, nullptr, nullptr, (gpk_layout*)b[kLayouts].p};
    gpk_tcp_streams as{};
    as.chunks = (gpk_tcp_chunk*)b[kChunks].p;
    as.stream_first = (uint32_t*)b[kFirst].p;
    as.stream_closed = (uint32_t*)b[kClosed].p;
    as.stream_data0 = (uint64_t*)b[kData0].p;
    as.counts = (uint64_t*)b[kAsmCounts].p;
    as.data = b[kAsmData].p;
    as.chunk_cap = s[1];
    as.data_cap = s[2];
    gpk_dns_stream_in in{(const uint32_t*)b[kInState].p, (const uint64_t*)b[kInOff].p, (const uint32_t*)b[kInLen].p,
                         b[kInTails].n ? b[kInTails].p : nullptr, s[3], b[kInTails].n, (uint32_t)s[4], (uint32_t)s[6]};
    Block o[kBlocks];
    for (int k = kStreams; k < kBlocks; k++) {
      o[k].n = b[k].n;
      o[k].p = (uint8_t*)malloc(o[k].n ? o[k].n : 1);
      memset(o[k].p, (int)fill, o[k].n);
    }
    gpk_dns_stream_out out{(gpk_dns_stream*)o[kStreams].p,
                           o[kMsgs].n ? (gpk_dns_stream_msg*)o[kMsgs].p : nullptr,
                           o[kRrs].n ? (gpk_dns_rr*)o[kRrs].p : nullptr,
                           o[kNames].n ? o[kNames].p : nullptr,
                           o[kTails].n ? o[kTails].p : nullptr,
                           (uint64_t*)o[kCounts].p,
                           o[kMsgs].n / sizeof(gpk_dns_stream_msg),
                           o[kRrs].n / sizeof(gpk_dns_rr),
                           o[kNames].n,
                           o[kTails].n};
    const int rc = gpk_dns_streams_host((const gpk_parser*)g_tables, &batch, &res, &as, &in, &out);
    if (rc != GPK_OK) {
      printf("call %u: rc %d\n", c, rc);
      bad++;
      continue;
    }
    for (int k = kStreams; k < kBlocks; k++)
      if (memcmp(o[k].p, b[k].p, b[k].n)) {
        printf("call %u: output %d differs from the model's\n", c, k - kStreams);
        bad++;
      }
  }
  fclose(f);
  delete g_tables;
  if (bad) return 1;
  printf("dns_streams_host ok: %u calls\n", ncalls);
  return 0;
}
