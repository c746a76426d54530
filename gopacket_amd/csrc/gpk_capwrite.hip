// gpk_capwrite.hip — pcap and pcapng writers (include/gpk_capwrite.h): the
// blocks that are not packets are built on the host; the packets of a device
// batch are framed on the device.
//
//   1. size_kernel    one lane per output packet: the reference's checks in its
//                     order, the block's size (0 for a packet in error) and the
//                     status
//   2. hipcub scan    exclusive sum of the sizes in uint64: block_off[0..m]
//   3. counts_kernel  blocks written, bytes needed, packets in error, overflow
//   4. frame_kernel   one group of G lanes per output packet, G = 64 (one wave)
//                     or 16 (four packets per wave, for batches of small
//                     blocks). The data moves with gpk_copy.h's copy_bytes<G>:
//                     destination-aligned 16-byte stores, the source realigned
//                     from two aligned 16-byte loads, a byte head and tail. The
//                     64-lane form switches on the source's dword phase, which
//                     is wave-uniform there; in the 16-lane form the four
//                     packets of a wave have four phases, so it selects the five
//                     words it needs instead of branching. The packet head, the
//                     padding and the trailing length are computed in registers
//                     by every lane and stored by the first lanes of the group,
//                     as dwords where the block starts on a dword, else as
//                     bytes. No cross-lane operation is used, so nothing needs
//                     uniform control flow; no per-lane array is indexed at run
//                     time, so there is no scratch.
// The host version (gpk_capwrite_batch_host) runs the same plan and head
// functions in a loop.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <new>

#include "../../include/gpk_capwrite.h"
#include "gpk_copy.h"
#include "gpk_devguard.h"
#include "gpk_scan.h"

namespace {

constexpr uint32_t kNgHead = 28, kPcapHead = 16;
constexpr uint64_t kNanos = 1000000000ull;
// batches whose mean block is at most this many bytes take the 16-lane framing kernel.
// Measured (tools/capwrite_bench.py, profiles/capwrite.json): 16 lanes
// per packet win up to blocks of 1532 bytes, 64 lanes from 2080 bytes on.
constexpr uint64_t kGroup16MaxMean = 1792;

struct Head {
  uint32_t h0, h1, h2, h3, h4, h5, h6;
};

// The checks of WritePacket / WritePacketWithOptions in their order and the
// block's size. i = the packet in the batch, optlen = its encoded options.
__host__ __device__ inline int32_t plan_block(int format, uint32_t interfaces, uint64_t n, uint64_t i,
                                              const uint32_t* caplens, const gpk_capture_info* ci, uint64_t optlen,
                                              uint32_t* size) {
  *size = 0;
  if (i >= n) return GPK_CAPW_EINDEX;
  const uint32_t caplen = caplens[i];
  const uint32_t length = ci[i].length;
  uint64_t total;
  if (format == GPK_CAPW_PCAPNG) {
    const int32_t iface = ci[i].iface;
    if (iface < 0 || (uint32_t)iface >= interfaces) return GPK_CAPW_EIFACE;
    if (caplen > length) return GPK_CAPW_ELENGTH;
    total = (uint64_t)kNgHead + caplen + ((4 - (caplen & 3)) & 3) + optlen + 4;
  } else {
    if (caplen > length) return GPK_CAPW_ELENGTH;
    total = (uint64_t)kPcapHead + caplen;
  }
  if (total >> 32) return GPK_CAPW_EBIG;
  *size = (uint32_t)total;
  return GPK_CAPW_OK;
}

__host__ __device__ inline Head make_head(int format, const gpk_capture_info& c, uint32_t caplen, uint32_t size,
                                          int64_t now_sec, uint32_t now_nsec) {
  Head h;
  if (format == GPK_CAPW_PCAPNG) {
    const uint64_t ts = (uint64_t)c.ts_sec * kNanos + c.ts_nsec;  // Time.UnixNano: wraps
    h = Head{6u, size, (uint32_t)c.iface, (uint32_t)(ts >> 32), (uint32_t)ts, caplen, c.length};
  } else {
    int64_t sec = c.ts_sec + (int64_t)(c.ts_nsec / (uint32_t)kNanos);  // time.Unix normalises
    uint32_t nsec = c.ts_nsec % (uint32_t)kNanos;
    if (sec == GPK_CAPW_ZERO_TIME_SEC && nsec == 0) {  // t.IsZero(): time.Now()
      sec = now_sec;
      nsec = now_nsec;
    }
    h = Head{(uint32_t)sec, format == GPK_CAPW_PCAP_MICRO ? nsec / 1000u : nsec, caplen, c.length, 0u, 0u, 0u};
  }
  return h;
}

__host__ __device__ inline uint32_t head_word(const Head& h, uint32_t k) {
  return k == 0 ? h.h0 : k == 1 ? h.h1 : k == 2 ? h.h2 : k == 3 ? h.h3 : k == 4 ? h.h4 : k == 5 ? h.h5 : h.h6;
}

struct SizeArgs {
  int format;
  uint32_t interfaces;
  uint64_t n, m;
  const uint32_t* caplens;
  const uint32_t* order;
  const gpk_capture_info* ci;
  const uint64_t* opt_off;
  uint32_t* bsize;  // [m + 1], bsize[m] = 0: the scan's last output is the total
  int32_t* status;
};

__global__ void __launch_bounds__(256) size_kernel(SizeArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > a.m) return;
  if (j == a.m) {
    a.bsize[j] = 0;
    return;
  }
  const uint64_t i = a.order ? a.order[j] : j;
  const uint64_t optlen = a.opt_off && a.format == GPK_CAPW_PCAPNG ? a.opt_off[j + 1] - a.opt_off[j] : 0;
  uint32_t size;
  a.status[j] = plan_block(a.format, a.interfaces, a.n, i, a.caplens, a.ci, optlen, &size);
  a.bsize[j] = size;
}

using SizeIt = hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*>;

__global__ void __launch_bounds__(256) counts_kernel(const int32_t* status, const uint64_t* block_off, uint64_t m,
                                                     uint64_t cap, uint64_t* counts) {
  // a fixed grid strides over the packets; one atomic pair per wave at the end
  uint32_t wrote = 0, errors = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    const int32_t st = status[j];
    wrote += st == GPK_CAPW_OK && block_off[j + 1] <= cap;
    errors += st != GPK_CAPW_OK;
    if (j + 1 == m) {
      counts[1] = block_off[m];
      counts[3] = block_off[m] > cap;
    }
  }
  for (int k = 32; k; k >>= 1) {  // every lane of the wave is here
    wrote += (uint32_t)__shfl_xor((int)wrote, k);
    errors += (uint32_t)__shfl_xor((int)errors, k);
  }
  if ((threadIdx.x & 63) == 0) {
    if (wrote) atomicAdd((unsigned long long*)&counts[0], (unsigned long long)wrote);
    if (errors) atomicAdd((unsigned long long*)&counts[2], (unsigned long long)errors);
  }
}

struct FrameArgs {
  int format;
  uint64_t m;
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* caplens;
  const uint32_t* order;
  const gpk_capture_info* ci;
  const uint8_t* opt_data;
  const uint64_t* opt_off;
  const uint64_t* block_off;
  uint8_t* out;
  uint64_t cap;
  int64_t now_sec;
  uint32_t now_nsec;
};

template <int G>
__global__ void __launch_bounds__(256) frame_kernel(FrameArgs a) {
  constexpr uint32_t kPerBlock = 256 / G;
  const uint32_t lane = threadIdx.x & (G - 1);
  const uint64_t stride = (uint64_t)gridDim.x * kPerBlock;
  const bool ng = a.format == GPK_CAPW_PCAPNG;
  const uint32_t hbytes = ng ? kNgHead : kPcapHead;
  for (uint64_t j = (uint64_t)blockIdx.x * kPerBlock + threadIdx.x / G; j < a.m; j += stride) {
    const uint64_t at = a.block_off[j], end = a.block_off[j + 1];
    // a packet in error has no bytes; a block that does not fit is not written at all
    if (end == at || end > a.cap) continue;
    const uint32_t size = (uint32_t)(end - at);
    const uint64_t i = a.order ? a.order[j] : j;  // in range: the size kernel gave this packet a size
    const uint32_t caplen = a.caplens[i];
    const Head h = make_head(a.format, a.ci[i], caplen, size, a.now_sec, a.now_nsec);
    uint8_t* dst = a.out + at;
    if (((uintptr_t)dst & 3) == 0) {
      if (lane < hbytes / 4) ((uint32_t*)dst)[lane] = head_word(h, lane);
    } else {
      for (uint32_t b = lane; b < hbytes; b += G) dst[b] = (uint8_t)(head_word(h, b >> 2) >> ((b & 3) * 8));
    }
    gpk::copy_bytes<G>(dst + hbytes, a.data + a.offsets[i], caplen, lane);
    if (!ng) continue;
    const uint32_t pad = (4 - (caplen & 3)) & 3;
    uint8_t* t = dst + kNgHead + caplen;
    if (lane < pad) t[lane] = 0;
    t += pad;
    const uint32_t optlen = size - kNgHead - caplen - pad - 4;
    if (optlen) gpk::copy_bytes<G>(t, a.opt_data + a.opt_off[j], optlen, lane);
    t += optlen;
    if (((uintptr_t)t & 3) == 0) {
      if (lane == 0) *(uint32_t*)t = size;
    } else if (lane < 4) {
      t[lane] = (uint8_t)(size >> (lane * 8));
    }
  }
}

// ---- host blocks
struct Sink {  // counts always, writes when it has a buffer
  uint8_t* p;
  uint64_t n = 0;
  explicit Sink(uint8_t* out) : p(out) {}
  void put(const void* s, uint64_t len) {
    if (p && len) memcpy(p + n, s, len);
    n += len;
  }
  void zeros(uint64_t len) {
    if (p && len) memset(p + n, 0, len);
    n += len;
  }
  void u16(uint16_t v) {
    const uint8_t b[2] = {(uint8_t)v, (uint8_t)(v >> 8)};
    put(b, 2);
  }
  void u32(uint32_t v) {
    const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    put(b, 4);
  }
  void u64(uint64_t v) {
    u32((uint32_t)v);
    u32((uint32_t)(v >> 32));
  }
};

enum OptKind { kOptBytes, kOptFilter, kOptU64, kOptU8, kOptTime };
struct Opt {
  uint16_t code;
  OptKind kind;
  gpk_capw_bytes bytes;
  uint64_t value;
};

uint64_t opt_length(const Opt& o) {  // ngOptionLength
  switch (o.kind) {
    case kOptBytes: return o.bytes.len;
    case kOptFilter: return o.bytes.len + 1;
    case kOptU8: return 1;
    default: return 8;
  }
}

uint32_t opts_length(const Opt* o, int k) {  // prepareNgOptions, in uint32 like the reference
  uint32_t ret = 0;
  for (int i = 0; i < k; i++) {
    const uint64_t len = opt_length(o[i]);
    ret += (uint32_t)(len + ((4 - (len & 3)) & 3) + 4);
  }
  return ret ? ret + 4 : 0;
}

void write_opts(Sink& s, const Opt* o, int k) {  // writeOptions
  if (!k) return;
  for (int i = 0; i < k; i++) {
    const uint64_t len = opt_length(o[i]);
    s.u16(o[i].code);
    s.u16((uint16_t)len);  // option.length is a uint16
    switch (o[i].kind) {
      case kOptFilter:
        s.zeros(1);
        [[fallthrough]];
      case kOptBytes:
        s.put(o[i].bytes.data, o[i].bytes.len);
        s.zeros((4 - ((uint16_t)len & 3)) & 3);
        break;
      case kOptTime:  // uint32(ts >> 32), uint32(ts)
        s.u32((uint32_t)(o[i].value >> 32));
        s.u32((uint32_t)o[i].value);
        break;
      case kOptU64: s.u64(o[i].value); break;
      case kOptU8: s.u32((uint32_t)(o[i].value & 0xFF)); break;
    }
  }
  s.u32(0);  // end of options
}

bool is_zero_time(int64_t sec, uint32_t nsec) { return sec == GPK_CAPW_ZERO_TIME_SEC && nsec == 0; }
uint64_t unix_nano(int64_t sec, uint32_t nsec) { return (uint64_t)sec * kNanos + nsec; }

template <class F>
int emit(uint8_t* out, uint64_t cap, F&& build) {
  Sink count(nullptr);
  build(count);
  if (count.n > 0x7FFFFFFFull) return GPK_EINVAL;
  if (count.n <= cap && out) {
    Sink w(out);
    build(w);
  }
  return (int)count.n;
}

}  // namespace

struct gpk_capwriter {
  int format = 0;
  int device = -1;
  uint32_t interfaces = 0;
  uint64_t cap = 0;
  uint32_t* bsize = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
};

extern "C" int gpk_capwriter_create(gpk_capwriter** out, int format, int device, uint64_t max_packets) {
  if (!out || format < GPK_CAPW_PCAP_MICRO || format > GPK_CAPW_PCAPNG) return GPK_EINVAL;
  if (device >= 0 && (max_packets == 0 || max_packets >= (1ull << 31) - 1)) return GPK_EINVAL;
  gpk_capwriter* w = new (std::nothrow) gpk_capwriter();
  if (!w) return GPK_ENOMEM;
  w->format = format;
  if (device >= 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
      delete w;
      return GPK_ENODEV;
    }
    gpk::DeviceScope dscope(device);
    if (dscope.err != hipSuccess) {
      delete w;
      return GPK_EHIP;
    }
    w->device = device;
    w->cap = max_packets;
    size_t tb = 0;
    bool ok = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, SizeIt(nullptr, Widen()), (uint64_t*)nullptr,
                                               (int)(max_packets + 1)) == hipSuccess;
    w->tmp_bytes = std::max(tb, (size_t)16);
    ok = ok && hipMalloc((void**)&w->bsize, (max_packets + 1) * 4) == hipSuccess &&
         hipMalloc(&w->tmp, w->tmp_bytes) == hipSuccess;
    if (!ok) {
      if (w->bsize) (void)hipFree(w->bsize);
      if (w->tmp) (void)hipFree(w->tmp);
      delete w;
      return GPK_ENOMEM;
    }
  }
  *out = w;
  return GPK_OK;
}

extern "C" int gpk_capwriter_destroy(gpk_capwriter* w) {
  if (!w) return GPK_EINVAL;
  if (w->device >= 0) {
    gpk::DeviceScope dscope(w->device);
    (void)hipDeviceSynchronize();
    if (w->bsize) (void)hipFree(w->bsize);
    if (w->tmp) (void)hipFree(w->tmp);
  }
  delete w;
  return GPK_OK;
}

extern "C" int gpk_capwriter_interfaces(const gpk_capwriter* w) {
  if (!w) return GPK_EINVAL;
  return (int)std::min<uint32_t>(w->interfaces, 0x7FFFFFFFu);
}

extern "C" int gpk_capwriter_set_interfaces(gpk_capwriter* w, uint32_t n) {
  if (!w || w->format != GPK_CAPW_PCAPNG) return GPK_EINVAL;
  w->interfaces = n;
  return GPK_OK;
}

extern "C" int gpk_capwrite_file_header(const gpk_capwriter* w, uint32_t snaplen, uint32_t link_type, uint8_t* out,
                                        uint64_t cap) {
  if (!w || w->format == GPK_CAPW_PCAPNG) return GPK_EINVAL;
  const uint32_t magic = w->format == GPK_CAPW_PCAP_MICRO ? 0xA1B2C3D4u : 0xA1B23C4Du;
  return emit(out, cap, [&](Sink& s) {
    s.u32(magic);
    s.u16(2);
    s.u16(4);
    s.u64(0);  // timezone, sigfigs
    s.u32(snaplen);
    s.u32(link_type);
  });
}

extern "C" int gpk_capwrite_section_header(const gpk_capwriter* w, const gpk_capw_section* info, uint8_t* out,
                                           uint64_t cap) {
  if (!w || !info || w->format != GPK_CAPW_PCAPNG) return GPK_EINVAL;
  Opt o[4];
  int k = 0;
  if (info->application.len) o[k++] = Opt{4, kOptBytes, info->application, 0};
  if (info->comment.len) o[k++] = Opt{1, kOptBytes, info->comment, 0};
  if (info->hardware.len) o[k++] = Opt{2, kOptBytes, info->hardware, 0};
  if (info->os.len) o[k++] = Opt{3, kOptBytes, info->os, 0};
  const uint32_t length = opts_length(o, k) + 24 + 4;
  return emit(out, cap, [&](Sink& s) {
    s.u32(0x0A0D0D0Au);
    s.u32(length);
    s.u32(0x1A2B3C4Du);
    s.u16(1);
    s.u16(0);
    s.u64(0xFFFFFFFFFFFFFFFFull);  // section length: unspecified
    write_opts(s, o, k);
    s.u32(length);
  });
}

extern "C" int gpk_capwrite_add_interface(gpk_capwriter* w, const gpk_capw_interface* f, uint8_t* out, uint64_t cap,
                                          int* id) {
  if (!w || !f || w->format != GPK_CAPW_PCAPNG) return GPK_EINVAL;
  Opt o[7];
  int k = 0;
  if (f->name.len) o[k++] = Opt{2, kOptBytes, f->name, 0};
  if (f->comment.len) o[k++] = Opt{1, kOptBytes, f->comment, 0};
  if (f->description.len) o[k++] = Opt{3, kOptBytes, f->description, 0};
  if (f->filter.len) o[k++] = Opt{11, kOptFilter, f->filter, 0};
  if (f->os.len) o[k++] = Opt{12, kOptBytes, f->os, 0};
  if (f->ts_offset) o[k++] = Opt{14, kOptU64, {nullptr, 0}, f->ts_offset};
  o[k++] = Opt{9, kOptU8, {nullptr, 0}, 9};  // nanoseconds, to match time.Time
  const uint32_t length = opts_length(o, k) + 16 + 4;
  const int n = emit(out, cap, [&](Sink& s) {
    s.u32(1);
    s.u32(length);
    s.u16(f->link_type);
    s.u16(0);
    s.u32(f->snap_length);
    write_opts(s, o, k);
    s.u32(length);
  });
  if (n > 0 && out && (uint64_t)n <= cap) {
    if (id) *id = (int)w->interfaces;
    w->interfaces++;
  }
  return n;
}

extern "C" int gpk_capwrite_interface_stats(const gpk_capwriter* w, int64_t intf, const gpk_capw_stats* st,
                                            uint8_t* out, uint64_t cap) {
  if (!w || !st || w->format != GPK_CAPW_PCAPNG) return GPK_EINVAL;
  if (intf >= (int64_t)w->interfaces || intf < 0) return GPK_CAPW_EIFACE;
  Opt o[4];
  int k = 0;
  if (!is_zero_time(st->start_time_sec, st->start_time_nsec))
    o[k++] = Opt{2, kOptTime, {nullptr, 0}, unix_nano(st->start_time_sec, st->start_time_nsec)};
  if (!is_zero_time(st->end_time_sec, st->end_time_nsec))
    o[k++] = Opt{3, kOptTime, {nullptr, 0}, unix_nano(st->end_time_sec, st->end_time_nsec)};
  if (st->packets_dropped != ~0ull) o[k++] = Opt{5, kOptU64, {nullptr, 0}, st->packets_dropped};
  if (st->packets_received != ~0ull) o[k++] = Opt{4, kOptU64, {nullptr, 0}, st->packets_received};
  const uint32_t length = opts_length(o, k) + 24;
  const uint64_t ts =
      is_zero_time(st->last_update_sec, st->last_update_nsec) ? 0 : unix_nano(st->last_update_sec, st->last_update_nsec);
  return emit(out, cap, [&](Sink& s) {
    s.u32(5);
    s.u32(length);
    s.u32((uint32_t)intf);
    s.u32((uint32_t)(ts >> 32));
    s.u32((uint32_t)ts);
    write_opts(s, o, k);
    s.u32(length);
  });
}

extern "C" int gpk_capwrite_secrets(const gpk_capwriter* w, uint32_t type, const uint8_t* payload, uint64_t len,
                                    uint8_t* out, uint64_t cap) {
  if (!w || w->format != GPK_CAPW_PCAPNG || (len && !payload)) return GPK_EINVAL;
  switch (type) {
    case 0x5353484bu:  // SSH
    case 0x5a4e574bu:  // Zigbee NWK
    case 0x57474b4cu:  // WireGuard
    case 0x5a415053u:  // Zigbee APS
    case 0x544c534bu:  // TLS
      break;
    default: return GPK_CAPW_ESECRETS;
  }
  const uint64_t pad = (4 - (len & 3)) & 3;
  const uint32_t length = (uint32_t)(8 + 4 + 8 + len + pad);
  return emit(out, cap, [&](Sink& s) {
    s.u32(10);
    s.u32(length);
    s.u32(type);
    s.u32((uint32_t)len);
    s.put(payload, len);
    s.zeros(pad);
    s.u32(length);
  });
}

namespace {

bool batch_args_ok(const gpk_capwriter* w, const gpk_batch* b, uint64_t m, const gpk_capture_info* ci,
                   const uint8_t* opt_data, const uint64_t* opt_off, uint8_t* out, uint64_t out_cap,
                   uint64_t* block_off, int32_t* status, uint64_t* counts) {
  if (!w || !b || !block_off || !counts) return false;
  if (m && (!status || !ci || !b->caplens || !b->offsets || !b->data)) return false;
  if ((opt_data == nullptr) != (opt_off == nullptr)) return false;
  if (out_cap && !out) return false;
  return true;
}

}  // namespace

extern "C" int gpk_capwrite_batch_host(gpk_capwriter* w, const gpk_batch* b, const uint32_t* order, uint64_t m,
                                       const gpk_capture_info* ci, const uint8_t* opt_data, const uint64_t* opt_off,
                                       const gpk_capwrite_opts* opts, uint8_t* out, uint64_t out_cap,
                                       uint64_t* block_off, int32_t* status, uint64_t* counts) {
  if (!batch_args_ok(w, b, m, ci, opt_data, opt_off, out, out_cap, block_off, status, counts)) return GPK_EINVAL;
  const int64_t now_sec = opts ? opts->now_sec : 0;
  const uint32_t now_nsec = opts ? opts->now_nsec : 0;
  const bool ng = w->format == GPK_CAPW_PCAPNG;
  uint64_t at = 0, written = 0, errors = 0;
  block_off[0] = 0;
  for (uint64_t j = 0; j < m; j++) {
    const uint64_t i = order ? order[j] : j;
    const uint64_t optlen = opt_off && ng ? opt_off[j + 1] - opt_off[j] : 0;
    uint32_t size;
    status[j] = plan_block(w->format, w->interfaces, b->n, i, b->caplens, ci, optlen, &size);
    if (status[j] != GPK_CAPW_OK) errors++;
    if (size && at + size <= out_cap) {
      const uint32_t caplen = b->caplens[i];
      const Head h = make_head(w->format, ci[i], caplen, size, now_sec, now_nsec);
      Sink s(out + at);
      for (uint32_t k = 0; k < (ng ? kNgHead : kPcapHead) / 4; k++) s.u32(head_word(h, k));
      s.put(b->data + b->offsets[i], caplen);
      if (ng) {
        s.zeros((4 - (caplen & 3)) & 3);
        if (optlen) s.put(opt_data + opt_off[j], optlen);
        s.u32(size);
      }
      written++;
    }
    at += size;
    block_off[j + 1] = at;
  }
  counts[0] = written;
  counts[1] = at;
  counts[2] = errors;
  counts[3] = at > out_cap;
  return GPK_OK;
}

extern "C" int gpk_capwrite_batch(gpk_capwriter* w, const gpk_batch* b, const uint32_t* order, uint64_t m,
                                  const gpk_capture_info* ci, const uint8_t* opt_data, const uint64_t* opt_off,
                                  const gpk_capwrite_opts* opts, uint8_t* out, uint64_t out_cap, uint64_t* block_off,
                                  int32_t* status, uint64_t* counts, void* stream) {
  if (!batch_args_ok(w, b, m, ci, opt_data, opt_off, out, out_cap, block_off, status, counts)) return GPK_EINVAL;
  if (w->device < 0 || m > w->cap) return GPK_EINVAL;
  const uint32_t group = opts ? opts->group : 0;
  if (group != 0 && group != 16 && group != 64) return GPK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  gpk::DeviceScope dscope(w->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (hipMemsetAsync(counts, 0, 4 * sizeof(uint64_t), s) != hipSuccess) return GPK_EHIP;
  if (m == 0) return hipMemsetAsync(block_off, 0, sizeof(uint64_t), s) == hipSuccess ? GPK_OK : GPK_EHIP;
  const dim3 blk(256);
  const SizeArgs sa{w->format, w->interfaces, b->n, m, b->caplens, order, ci, opt_off, w->bsize, status};
  hipLaunchKernelGGL(size_kernel, dim3((unsigned)((m + 1 + 255) / 256)), blk, 0, s, sa);
  size_t tb = w->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(w->tmp, tb, SizeIt(w->bsize, Widen()), block_off, (int)(m + 1), s) !=
      hipSuccess)
    return GPK_EHIP;
  hipLaunchKernelGGL(counts_kernel, dim3((unsigned)std::min<uint64_t>((m + 255) / 256, 2048)), blk, 0, s, status,
                     block_off, m, out_cap, counts);
  const FrameArgs fa{w->format, m,  b->data,   b->offsets, b->caplens, order,
                     ci,        opt_data, opt_off, block_off,  out,        out_cap,
                     opts ? opts->now_sec : 0, opts ? opts->now_nsec : 0};
  // the mean block size, from the batch's mean packet size (data_bytes as in gpk_decode_batch: a hint)
  const uint64_t mean = (b->n && b->data_bytes ? b->data_bytes / b->n : kGroup16MaxMean + 1) +
                        (w->format == GPK_CAPW_PCAPNG ? 32 : 16);
  const bool small = group ? group == 16 : mean <= kGroup16MaxMean;
  if (small) {
    const uint64_t want = (m + 15) / 16;  // 16 groups per block, one packet per group per pass
    hipLaunchKernelGGL(frame_kernel<16>, dim3((unsigned)std::min<uint64_t>(want, 65536)), blk, 0, s, fa);
  } else {
    const uint64_t want = (m + 3) / 4;  // 4 waves per block, one packet per wave per pass
    hipLaunchKernelGGL(frame_kernel<64>, dim3((unsigned)std::min<uint64_t>(want, 65536)), blk, 0, s, fa);
  }
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}
