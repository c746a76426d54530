// gpk_dns_streams.hip — the DNS messages of reassembled TCP streams
// (include/gpk_dns_streams.h): the step between gpk_tcpasm_batch's
// contiguous stream bytes and the message rules of gpk_dns_rules.h. Framing and
// decoding are separate steps: one lane per stream only chases length prefixes,
// and the decode runs with one lane per message.
//
//   init_kernel, cut_kernel (gpk_streams.h, as the tail_kernel and the stream's
//                 View): where each stream's logical buffer is cut, and whether
//                 it has a start
//   count_kernel  one lane per stream: candidate, carried state, then the chase
//                 over the length prefixes, two bytes per message and no decode;
//                 the stream entry with its state, nmsg, consumed and tail_len
//   scan          exclusive sums of (messages, tail bytes, streams framed) over
//                 the streams
//   place_kernel  one lane per stream: msg0 and tail_off; the chase again, which
//                 writes {stream, hdr_off, len, status, present} of its messages
//                 when the stream's range fits msg_cap and tail_cap; the last
//                 stream writes the stream-level counts
//   size_kernel   one lane per placed message: walk<false>, the gpk_dns record
//   scan          exclusive sums of (rr entries, name bytes, failed) over the
//                 message entries
//   emit_kernel   one lane per placed message: rr0 and name0; walk<true> when its
//                 range fits rr_cap and name_cap; the last message writes the
//                 message-level counts
//   tail_kernel   the unfinished tails into the tail arena
// The numbers of streams and of placed messages stay on the device: the grids
// over messages are sized by msg_cap and their lanes leave at the device count.
// Only a stream's first message can straddle the carried tail and the new
// bytes; it is decoded in place through gpk::Seam, every other message from a
// plain pointer.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <new>

#include "../../include/gpk_dns_streams.h"
#include "gpk_copy.h"
#include "gpk_devguard.h"
#include "gpk_dns_rules.h"
#include "gpk_seam.h"
#include "gpk_streams.h"
#include "gpk_workspace.h"

// gpk_host.cpp: the parser's tables in host memory, and a step enqueued on
// `stream` with their device copy (kept until it completes)
extern "C" __attribute__((visibility("hidden"))) const gpk::DevTables* gpk_parser_tables(const gpk_parser* p);
extern "C" __attribute__((visibility("hidden"))) int gpk_with_device_tables(
    gpk_ctx* c, const gpk_parser* p, void* stream, int (*step)(const gpk::DevTables*, void*), void* arg);

namespace {

// the pass as gpk_streams.h takes it
struct DnsPass {
  using In = gpk_dns_stream_in;
  using Out = gpk_dns_stream_out;
  using Stream = gpk_dns_stream;
  static constexpr int32_t kLayer = GPK_LT_DNS;
  static constexpr uint32_t kNew = GPK_DNSS_NEW, kSynced = GPK_DNSS_SYNCED, kNone = GPK_DNSS_NONE,
                            kNostart = GPK_DNSS_NOSTART, kNState = GPK_DNSS_NSTATE;
  static constexpr uint32_t kFrameUnstarted = GPK_DNSS_FRAME_UNSTARTED, kAllFlags = GPK_DNSS_ALL_FLAGS;
  static constexpr uint32_t kDropped = GPK_DNSS_ST_DROPPED, kTooBig = GPK_DNSS_ST_TOOBIG,
                            kBadTail = GPK_DNSS_ST_BADTAIL;
};

struct Args : StreamArgs<DnsPass> {
  uint64_t* placed;  // [1] message entries written by place: the device count of the grids over messages
};

// what lies in front of a stream: message entries, tail bytes, streams framed
struct STot {
  uint64_t msg, tail, framed;
};
struct STotAdd {
  __host__ __device__ STot operator()(const STot& a, const STot& b) const {
    return STot{a.msg + b.msg, a.tail + b.tail, a.framed + b.framed};
  }
};
GPK_HD STot own_of(const Args& a, uint32_t j) {
  const gpk_dns_stream& e = a.out.streams[j];
  return STot{e.nmsg, e.tail_len, a.framed[j]};
}
struct STotOf {  // of stream j; nothing past S
  Args a;
  __host__ __device__ STot operator()(uint32_t j) const {
    if (j >= stream_count(a)) return STot{0, 0, 0};
    return own_of(a, j);
  }
};
using STotIn = hipcub::TransformInputIterator<STot, STotOf, hipcub::CountingInputIterator<uint32_t>>;

// what lies in front of a message: rr entries, name bytes, failed messages
struct MTot {
  uint64_t rr, nb, failed;
};
struct MTotAdd {
  __host__ __device__ MTot operator()(const MTot& a, const MTot& b) const {
    return MTot{a.rr + b.rr, a.nb + b.nb, a.failed + b.failed};
  }
};
GPK_HD MTot own_of(const gpk_dns_stream_msg& e) { return MTot{e.msg.nrr, e.msg.name_bytes, e.msg.err != 0}; }
struct MTotOf {  // of message entry m; nothing past the placed ones
  const gpk_dns_stream_msg* msgs;
  const uint64_t* placed;
  __host__ __device__ MTot operator()(uint32_t m) const {
    if (m >= *placed) return MTot{0, 0, 0};
    return own_of(msgs[m]);
  }
};
using MTotIn = hipcub::TransformInputIterator<MTot, MTotOf, hipcub::CountingInputIterator<uint32_t>>;

GPK_HD uint32_t max_len(const Args& a) { return a.in.max_msg_len ? a.in.max_msg_len : 65535u; }

struct Framed {
  uint32_t state, consumed, tail_len, nmsg;
};

// What place leaves of message entry k: five dwords, so that the one lane of a
// long stream stores little per message. The size step reads them back and
// writes the rest of the entry.
GPK_HD void place_entry(gpk_dns_stream_msg* e, uint32_t j, uint32_t hdr_off, uint32_t len, uint32_t status,
                        uint32_t present) {
  uint32_t* w = reinterpret_cast<uint32_t*>(e);
  w[3] = hdr_off;
  w[4] = len;
  w[16] = j;
  w[17] = status;
  w[18] = present;
}

// The chase over a stream's length prefixes (include/gpk_dns_streams.h).
// kPlace: entry k goes to msgs[k].
template <bool kPlace>
GPK_HD void chase(const View& v, uint32_t j, uint32_t cap, Framed& f, gpk_dns_stream_msg* msgs) {
  uint32_t off = 0, k = 0, length = 0;
  for (;;) {
    if (v.len - off < 2) break;
    if (off + 1 < v.tail_in) {
      length = gpk::tun::be16(v.tail + off);
    } else if (off < v.tail_in) {  // the prefix itself straddles the seam
      length = (uint32_t)v.tail[off] << 8 | v.nb[0];
    } else {
      length = gpk::tun::be16(v.nb + (off - v.tail_in));
    }
    if (v.len - off - 2 < length) break;
    if (kPlace) place_entry(msgs + k, j, off + 2, length, length > cap ? GPK_DNSS_MSG_SKIPPED : 0u, 2 + length);
    k++;
    off += 2 + length;
  }
  const uint32_t rest = v.len - off;
  uint32_t state = GPK_DNSS_SYNCED, tail_len = 0;
  if (v.lost || v.closed) {
    if (rest) {  // io.ReadFull fails: nothing is decoded
      if (kPlace) place_entry(msgs + k, j, off + 2, rest >= 2 ? length : 0u, GPK_DNSS_MSG_PARTIAL, rest);
      k++;
    }
    state = v.lost ? GPK_DNSS_LOST : GPK_DNSS_CLOSED;
  } else {
    tail_len = rest;
  }
  f = Framed{state, off, tail_len, k};
}

// the count step of stream j
GPK_HD void count_one(const Args& a, uint32_t j) {
  View v;
  resolve(a, j, v);
  Framed f{v.state, 0, 0, 0};
  if (v.frame) chase<false>(v, j, max_len(a), f, nullptr);
  a.framed[j] = v.frame;
  uint32_t* w = reinterpret_cast<uint32_t*>(&a.out.streams[j]);
  w[0] = f.state | v.status << 8;
  w[1] = v.tail_in;
  w[2] = f.consumed;
  w[3] = f.tail_len;
  w[4] = w[5] = 0;
  w[6] = f.nmsg;
  for (int k = 7; k < 16; k++) w[k] = 0;
}

GPK_HD bool fits(const gpk_dns_stream_out& o, const STot& t) { return t.msg <= o.msg_cap && t.tail <= o.tail_cap; }

// *p = max(*p, v) and *p += 1: by many lanes on the device, by the one thread on the host
GPK_HD void raise(uint64_t* p, uint64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  atomicMax((unsigned long long*)p, (unsigned long long)v);
#else
  if (v > *p) *p = v;
#endif
}
GPK_HD void bump(uint32_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
  atomicAdd(p, 1u);
#else
  ++*p;
#endif
}

// The place step of stream j (< S), t: the totals in front of it. The sums grow
// with j, so the streams that fit are the first ones and their entries are
// msgs[0 .. placed), placed being the largest end of a range that was written.
// The last stream also reports the stream-level totals. Returns whether the
// stream's tail is to be copied.
GPK_HD bool place_one(const Args& a, uint32_t j, uint32_t S, const STot& t) {
  gpk_dns_stream* e = &a.out.streams[j];
  const STot own = own_of(a, j), end = STotAdd()(t, own);
  if (j == S - 1) {
    uint64_t* c = a.out.counts;
    c[0] = S, c[1] = end.framed, c[2] = end.msg;
    c[4] = !fits(a.out, end);
    c[5] = end.msg, c[8] = end.tail;
  }
  e->msg0 = t.msg;
  e->tail_off = t.tail;
  if (!a.framed[j]) return false;
  if (!fits(a.out, end)) {
    e->status |= GPK_DNSS_ST_DROPPED;
    return false;
  }
  if (own.msg) {
    View v;
    resolve(a, j, v);
    Framed f;
    chase<true>(v, j, max_len(a), f, a.out.msgs + t.msg);
    raise(a.placed, end.msg);
  }
  return own.tail != 0;
}

// DecodeFromBytes on the message at hdr_off of stream j's logical buffer
template <bool kEmit>
GPK_HD void decode(const Args& a, uint32_t j, uint32_t hdr_off, uint32_t len, gpk::dns::Msg& msg, gpk_dns_rr* rrs,
                   uint8_t* names, uint64_t name0) {
  const uint32_t tail_in = a.out.streams[j].tail_in;
  const uint8_t* nb = a.as.data + a.as.stream_data0[j];
  if (hdr_off < tail_in) {  // the stream's first message, over the seam; tail_in > 0: j < in.n
    const gpk::Seam sm{a.in.tails + a.in.tail_off[j], nb, tail_in, hdr_off};
    gpk::dns::walk<kEmit>(sm, len, msg, rrs, names, name0);
  } else {
    gpk::dns::walk<kEmit>(nb + (hdr_off - tail_in), len, msg, rrs, names, name0);
  }
}

// the size step of message entry m (< placed)
GPK_HD void size_one(const Args& a, uint64_t m) {
  gpk_dns_stream_msg* e = &a.out.msgs[m];
  const uint32_t j = e->stream, len = e->msg.len;
  gpk::dns::Msg msg;
  gpk::dns::msg_init(msg, e->msg.hdr_off);
  if (e->status) {  // PARTIAL, SKIPPED: not decoded
    msg.len = len;
  } else {
    decode<false>(a, j, msg.hdr_off, len, msg, nullptr, nullptr, 0);
    if (msg.err) bump(&a.out.streams[j].nfailed);
  }
  gpk::dns::msg_store(&e->msg, msg);
  e->reserved2 = 0;
}

// The emit step of message entry m (< M = placed), t: the totals in front of it.
// The last entry also reports the message-level totals.
GPK_HD void emit_one(const Args& a, uint64_t m, uint64_t M, const MTot& t) {
  gpk_dns_stream_msg* e = &a.out.msgs[m];
  const MTot end = MTotAdd()(t, own_of(*e));
  if (m == M - 1) {
    uint64_t* c = a.out.counts;
    c[3] = end.failed;
    if (end.rr > a.out.rr_cap || end.nb > a.out.name_cap) c[4] = 1;
    c[6] = end.rr, c[7] = end.nb;
  }
  if (e->status || e->msg.err) return;
  e->msg.rr0 = t.rr;
  e->msg.name0 = t.nb;
  if (end.rr > a.out.rr_cap || end.nb > a.out.name_cap) {
    reinterpret_cast<uint32_t*>(e)[17] = GPK_DNSS_MSG_DROPPED;
    return;
  }
  gpk::dns::Msg msg;
  gpk::dns::msg_init(msg, e->msg.hdr_off);
  decode<true>(a, e->stream, e->msg.hdr_off, e->msg.len, msg, a.out.rrs + t.rr, a.out.names, t.nb);
}

__global__ void __launch_bounds__(kBlk) count_kernel(const Args a) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < stream_count(a)) count_one(a, (uint32_t)j);
}

__global__ void __launch_bounds__(kBlk) place_kernel(const Args a, const STot* starts) {
  const uint32_t S = stream_count(a);
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < S) place_one(a, (uint32_t)j, S, starts[j]);
}

__global__ void __launch_bounds__(kBlk) size_kernel(const Args a) {
  const uint64_t m = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (m < *a.placed) size_one(a, m);
}

__global__ void __launch_bounds__(kBlk) emit_kernel(const Args a, const MTot* starts) {
  const uint64_t M = *a.placed;
  const uint64_t m = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (m < M) emit_one(a, m, M, starts[m]);
}

bool bad_out(const gpk_dns_stream_out* o) {
  return !o || !o->streams || !o->counts || ((uintptr_t)o->streams & 7) || ((uintptr_t)o->msgs & 7) ||
         ((uintptr_t)o->rrs & 7) || (o->msg_cap && !o->msgs) || (o->rr_cap && !o->rrs) ||
         (o->name_cap && !o->names) || (o->tail_cap && !o->tails) || o->msg_cap >= (1ull << 28);
}

bool bad_args(const gpk_parser* p, const gpk_batch* b, const gpk_results* r, const gpk_tcp_streams* as,
              const gpk_dns_stream_in* in, const gpk_dns_stream_out* o) {
  return bad_out(o) || bad_stream_args<DnsPass>(p, b, r, as, in) || (in && in->max_msg_len > 65535u);
}

Args dns_args(const gpk_batch* b, const gpk_results* r, const gpk_tcp_streams* as, const gpk_dns_stream_in* in,
              const gpk_dns_stream_out* o) {
  Args a{};
  static_cast<StreamArgs<DnsPass>&>(a) = make_args<DnsPass>(b, r, as, in, o);
  return a;
}

}  // namespace

struct gpk_dns_stream_decoder {
  int device = 0;
  uint64_t cap = 0, msg_cap = 0;
  uint64_t* cut = nullptr;      // [cap]
  uint32_t* nostart = nullptr;  // [cap]
  uint32_t* framed = nullptr;   // [cap]
  STot* sstarts = nullptr;      // [cap]
  MTot* mstarts = nullptr;      // [msg_cap]
  uint64_t* placed = nullptr;   // [1]
  uint8_t* tmp = nullptr;       // of either scan
  size_t stmp_bytes = 0, mtmp_bytes = 0;
  gpk::Workspace ws;
  void carve() {
    ws.take(cut, cap), ws.take(nostart, cap), ws.take(framed, cap), ws.take(sstarts, cap);
    ws.take(mstarts, msg_cap), ws.take(placed, 1);
    const size_t tb = stmp_bytes > mtmp_bytes ? stmp_bytes : mtmp_bytes;
    ws.take(tmp, tb ? tb : 4);
  }
};

extern "C" int gpk_dns_stream_decoder_create(gpk_dns_stream_decoder** out, int device, uint64_t max_streams,
                                             uint64_t max_msgs) {
  if (max_msgs == 0 || max_msgs >= (1ull << 28)) return GPK_EINVAL;
  if (const int rc = gpk::check_create(out, device, max_streams, 1ull << 28)) return rc;
  gpk::DeviceScope dscope(device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  gpk_dns_stream_decoder* h = new (std::nothrow) gpk_dns_stream_decoder();
  if (!h) return GPK_ENOMEM;
  h->device = device;
  h->cap = max_streams;
  h->msg_cap = max_msgs;
  const bool ok =
      hipcub::DeviceScan::ExclusiveScan(nullptr, h->stmp_bytes,
                                        STotIn(hipcub::CountingInputIterator<uint32_t>(0), STotOf{Args{}}),
                                        (STot*)nullptr, STotAdd(), STot{0, 0, 0}, (int)max_streams) == hipSuccess &&
      hipcub::DeviceScan::ExclusiveScan(nullptr, h->mtmp_bytes,
                                        MTotIn(hipcub::CountingInputIterator<uint32_t>(0), MTotOf{nullptr, nullptr}),
                                        (MTot*)nullptr, MTotAdd(), MTot{0, 0, 0}, (int)max_msgs) == hipSuccess;
  h->carve();
  if (!ok || !h->ws.alloc()) {
    delete h;
    return GPK_ENOMEM;
  }
  h->carve();
  *out = h;
  return GPK_OK;
}

extern "C" int gpk_dns_stream_decoder_destroy(gpk_dns_stream_decoder* d) {
  if (!d) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  (void)hipDeviceSynchronize();
  d->ws.release();
  delete d;
  return GPK_OK;
}

namespace {

struct Launch {
  gpk_dns_stream_decoder* h;
  Args a;
  hipStream_t s;
};

int launch_step(const gpk::DevTables* tab, void* arg) {
  Launch& l = *static_cast<Launch*>(arg);
  gpk_dns_stream_decoder* h = l.h;
  Args& a = l.a;
  hipStream_t s = l.s;
  a.tab = tab;
  const StreamArgs<DnsPass>& sa = a;
  const unsigned blocks = (unsigned)((a.n + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(init_kernel<DnsPass>, dim3(blocks), dim3(kBlk), 0, s, sa);
  if (a.as.chunk_cap) {
    const uint64_t cb = (a.as.chunk_cap + kBlk - 1) / kBlk;
    if (cb >= (1ull << 31)) return GPK_EINVAL;
    hipLaunchKernelGGL(cut_kernel<DnsPass>, dim3((unsigned)cb), dim3(kBlk), 0, s, sa);
  }
  hipLaunchKernelGGL(count_kernel, dim3(blocks), dim3(kBlk), 0, s, a);
  size_t tb = h->stmp_bytes;
  const STotIn sin(hipcub::CountingInputIterator<uint32_t>(0), STotOf{a});
  if (hipcub::DeviceScan::ExclusiveScan(h->tmp, tb, sin, h->sstarts, STotAdd(), STot{0, 0, 0}, (int)a.n, s) !=
      hipSuccess)
    return GPK_EHIP;
  hipLaunchKernelGGL(place_kernel, dim3(blocks), dim3(kBlk), 0, s, a, (const STot*)h->sstarts);
  if (a.out.msg_cap) {
    const unsigned mblocks = (unsigned)((a.out.msg_cap + kBlk - 1) / kBlk);
    hipLaunchKernelGGL(size_kernel, dim3(mblocks), dim3(kBlk), 0, s, a);
    tb = h->mtmp_bytes;
    const MTotIn min(hipcub::CountingInputIterator<uint32_t>(0), MTotOf{a.out.msgs, a.placed});
    if (hipcub::DeviceScan::ExclusiveScan(h->tmp, tb, min, h->mstarts, MTotAdd(), MTot{0, 0, 0}, (int)a.out.msg_cap,
                                          s) != hipSuccess)
      return GPK_EHIP;
    hipLaunchKernelGGL(emit_kernel, dim3(mblocks), dim3(kBlk), 0, s, a, (const MTot*)h->mstarts);
  }
  if (a.out.tail_cap) hipLaunchKernelGGL(tail_kernel<DnsPass>, dim3(blocks), dim3(kBlk), 0, s, sa);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

}  // namespace

extern "C" int gpk_dns_streams(gpk_dns_stream_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                               const gpk_results* r, const gpk_tcp_streams* as, const gpk_dns_stream_in* in,
                               const gpk_dns_stream_out* o, void* stream) {
  if (!d || !ctx || bad_args(parser, b, r, as, in, o) || b->n > d->cap || o->msg_cap > d->msg_cap) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(o->counts, 0, 12 * 8, s) != hipSuccess) return GPK_EHIP;
  if (b->n == 0) return GPK_OK;
  if (hipMemsetAsync(d->placed, 0, 8, s) != hipSuccess) return GPK_EHIP;
  Launch l{d, dns_args(b, r, as, in, o), s};
  l.a.cut = d->cut, l.a.nostart = d->nostart, l.a.framed = d->framed, l.a.placed = d->placed;
  return gpk_with_device_tables(ctx, parser, stream, launch_step, &l);
}

extern "C" int gpk_dns_streams_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r,
                                    const gpk_tcp_streams* as, const gpk_dns_stream_in* in,
                                    const gpk_dns_stream_out* o) {
  if (bad_args(parser, b, r, as, in, o)) return GPK_EINVAL;
  for (int k = 0; k < 12; k++) o->counts[k] = 0;
  if (b->n == 0) return GPK_OK;
  Args a = dns_args(b, r, as, in, o);
  a.tab = gpk_parser_tables(parser);
  const uint32_t S = stream_count(a);
  if (S == 0) return GPK_OK;
  uint64_t placed = 0;
  a.placed = &placed;
  a.cut = new (std::nothrow) uint64_t[S];
  a.nostart = new (std::nothrow) uint32_t[S];
  a.framed = new (std::nothrow) uint32_t[S];
  int rc = GPK_ENOMEM;
  if (a.cut && a.nostart && a.framed) {
    host_cut<DnsPass>(a, S);
    for (uint32_t j = 0; j < S; j++) count_one(a, j);
    STot t{0, 0, 0};
    for (uint32_t j = 0; j < S; j++) {
      const STot own = own_of(a, j);
      if (place_one(a, j, S, t)) host_tail<DnsPass>(a, j, t.tail);
      t = STotAdd()(t, own);
    }
    for (uint64_t m = 0; m < placed; m++) size_one(a, m);
    MTot mt{0, 0, 0};
    for (uint64_t m = 0; m < placed; m++) {
      const MTot own = own_of(o->msgs[m]);
      emit_one(a, m, placed, mt);
      mt = MTotAdd()(mt, own);
    }
    rc = GPK_OK;
  }
  delete[] a.cut;
  delete[] a.nostart;
  delete[] a.framed;
  return rc;
}
