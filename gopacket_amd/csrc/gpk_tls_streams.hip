// gpk_tls_streams.hip — the TLS records of reassembled TCP streams
// (include/gpk_tls_streams.h): the step between gpk_tcpasm_batch's
// contiguous stream bytes and the record rules of gpk_tls_rules.h.
//
//   init_kernel, cut_kernel (gpk_streams.h, as the tail_kernel and the stream's
//                 View): where each stream's logical buffer is cut, and whether
//                 it has a start
//   size_kernel   one lane per stream: candidate, carried state, then the
//                 framing walk in size mode; the stream entry with its state and
//                 sizes
//   scan          exclusive sums of (records, failed, hellos, server name bytes,
//                 tail bytes, streams framed) over the streams
//   emit_kernel   one lane per stream: the walk again, in store mode, when the
//                 stream's whole range fits every capacity; the last stream
//                 also writes counts
//   tail_kernel   the unfinished tails into the tail arena
// The framing chain is serial: a header's position depends on the Length in
// front of it. One lane walks a stream, at one dependent header read per
// record. Only a stream's first record can straddle the carried tail and the
// new bytes; it is decoded in place through gpk::tls::Seam, every other record
// from a plain pointer.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <new>

#include "../../include/gpk_tls_streams.h"
#include "gpk_copy.h"
#include "gpk_devguard.h"
#include "gpk_streams.h"
#include "gpk_tls_rules.h"
#include "gpk_workspace.h"

// gpk_host.cpp: the parser's tables in host memory, and a step enqueued on
// `stream` with their device copy (kept until it completes)
extern "C" __attribute__((visibility("hidden"))) const gpk::DevTables* gpk_parser_tables(const gpk_parser* p);
extern "C" __attribute__((visibility("hidden"))) int gpk_with_device_tables(
    gpk_ctx* c, const gpk_parser* p, void* stream, int (*step)(const gpk::DevTables*, void*), void* arg);

namespace {

// the pass as gpk_streams.h takes it
struct TlsPass {
  using In = gpk_tls_stream_in;
  using Out = gpk_tls_stream_out;
  using Stream = gpk_tls_stream;
  static constexpr int32_t kLayer = GPK_LT_TLS;
  static constexpr uint32_t kNew = GPK_TLSS_NEW, kSynced = GPK_TLSS_SYNCED, kNone = GPK_TLSS_NONE,
                            kNostart = GPK_TLSS_NOSTART, kNState = GPK_TLSS_NSTATE;
  static constexpr uint32_t kFrameUnstarted = GPK_TLSS_FRAME_UNSTARTED, kAllFlags = GPK_TLSS_ALL_FLAGS;
  static constexpr uint32_t kDropped = GPK_TLSS_ST_DROPPED, kTooBig = GPK_TLSS_ST_TOOBIG,
                            kBadTail = GPK_TLSS_ST_BADTAIL;
};
using Args = StreamArgs<TlsPass>;

// what lies in front of a stream: record entries, failed ones, hello entries,
// server name bytes, tail bytes, streams framed
struct Tot {
  uint64_t rec, failed, hello, sni, tail, framed;
};
struct TotAdd {
  __host__ __device__ Tot operator()(const Tot& a, const Tot& b) const {
    return Tot{a.rec + b.rec, a.failed + b.failed, a.hello + b.hello, a.sni + b.sni, a.tail + b.tail,
               a.framed + b.framed};
  }
};

GPK_HD Tot own_of(const Args& a, uint32_t j) {
  const gpk_tls_stream& e = a.out.streams[j];
  return Tot{e.nrec, e.nfailed, e.nhello, e.sni_bytes, e.tail_len, a.framed[j]};
}

struct TotOf {  // of stream j; nothing past S
  Args a;
  __host__ __device__ Tot operator()(uint32_t j) const {
    if (j >= stream_count(a)) return Tot{0, 0, 0, 0, 0, 0};
    return own_of(a, j);
  }
};
using TotIn = hipcub::TransformInputIterator<Tot, TotOf, hipcub::CountingInputIterator<uint32_t>>;

struct Framed {
  uint32_t state, consumed, tail_len, nrec, nfailed, nhello, sni_bytes;
};

// entry k of the stream: the part behind gpk_tls_rec; a failed entry's gpk_tls_rec too
GPK_HD void store_entry(gpk_tls_stream_rec* r, bool failed, uint32_t ct, uint32_t version, uint32_t length,
                        uint32_t body_off, uint32_t err, uint32_t a0, uint32_t a1, uint32_t j) {
  uint32_t* w = reinterpret_cast<uint32_t*>(r);
  if (failed) {
    w[0] = ct;
    w[1] = version | length << 16;
    w[2] = body_off;
    w[3] = GPK_TLS_NO_HELLO;
  }
  w[4] = err | (err && gpk::tls::truncates(err) ? GPK_TLS_ST_TRUNCATED : 0u) << 8;
  w[5] = a0;
  w[6] = a1;
  w[7] = j;
}

// The framing walk over a stream's logical buffer (include/gpk_tls_streams.h).
// kStore: entry k goes to recs[k], hello k to hellos[k], the names to snis + sni0 on.
template <bool kStore>
GPK_HD void frame(const View& v, uint32_t j, Framed& f, gpk_tls_stream_rec* recs, gpk_tls_hello* hellos,
                  uint8_t* snis, uint64_t sni0) {
  gpk::tls::Msg m;
  gpk::tls::msg_init(m, 0);
  uint32_t off = 0, k = 0, failed = 0, ct = 0, version = 0, length = 0;
  uint32_t state = GPK_TLSS_SYNCED;
  for (;;) {
    if (v.len - off < 5) break;
    const bool seam = off < v.tail_in;
    const gpk::tls::Seam sm{v.tail, v.nb, v.tail_in, off};
    const uint8_t* p = seam ? v.nb : v.nb + (off - v.tail_in);
    if (seam) {
      ct = sm[0], version = be16(sm + 1), length = be16(sm + 3);
    } else {
      ct = p[0], version = gpk::tun::be16(p + 1), length = gpk::tun::be16(p + 3);
    }
    if (ct < 20 || ct > 23) {
      if (kStore) store_entry(recs + k, true, ct, version, length, off + 5, GPK_TLS_ERR_RECORD_TYPE, 0, 0, j);
      k++, failed++;
      off += 5;
      state = GPK_TLSS_NOT_TLS;
      break;
    }
    if (v.len - off < 5 + length) break;
    uint32_t l2, a0, a1;
    gpk_tls_rec* dst = kStore ? &recs[k].rec : nullptr;
    const uint32_t e = seam ? gpk::tls::record<kStore>(sm, 5 + length, 5 + length, off + 5, m, j, dst, hellos, snis,
                                                       sni0, l2, a0, a1)
                            : gpk::tls::record<kStore>(p, 5 + length, 5 + length, off + 5, m, j, dst, hellos, snis,
                                                       sni0, l2, a0, a1);
    if (kStore) store_entry(recs + k, e != 0, ct, version, length, off + 5, e, a0, a1, j);
    k++;
    failed += e != 0;
    off += 5 + length;
  }
  const uint32_t rest = v.len - off;
  uint32_t tail_len = 0;
  if (state != GPK_TLSS_NOT_TLS) {
    if (v.lost || v.closed) {
      if (rest) {  // DecodeFromBytes(rest): :131-134 or :150-155
        const bool hdr = rest >= 5;
        if (kStore)
          store_entry(recs + k, true, hdr ? ct : 0, hdr ? version : 0, hdr ? length : 0, off + 5,
                      hdr ? GPK_TLS_ERR_LENGTH_MISMATCH : GPK_TLS_ERR_RECORD_SHORT, 0, 0, j);
        k++, failed++;
      }
      state = v.lost ? GPK_TLSS_LOST : GPK_TLSS_CLOSED;
    } else {
      tail_len = rest;
    }
  }
  f = Framed{state, off, tail_len, k, failed, m.nhello, (uint32_t)m.sni_bytes};
}

// the size step of stream j
GPK_HD void size_one(const Args& a, uint32_t j) {
  View v;
  resolve(a, j, v);
  Framed f{v.state, 0, 0, 0, 0, 0, 0};
  if (v.frame) frame<false>(v, j, f, nullptr, nullptr, nullptr, 0);
  a.framed[j] = v.frame;
  uint32_t* w = reinterpret_cast<uint32_t*>(&a.out.streams[j]);
  w[0] = f.state | v.status << 8;
  w[1] = v.tail_in;
  w[2] = f.consumed;
  w[3] = f.tail_len;
  w[4] = w[5] = 0;
  w[6] = f.nrec;
  w[7] = f.nfailed;
  w[8] = f.nhello;
  w[9] = f.sni_bytes;
  w[10] = w[11] = w[12] = w[13] = w[14] = w[15] = 0;
}

GPK_HD bool fits(const gpk_tls_stream_out& o, const Tot& t) {
  return t.rec <= o.rec_cap && t.hello <= o.hello_cap && t.sni <= o.sni_cap && t.tail <= o.tail_cap;
}

// The emit step of stream j (< S), t: the totals in front of it. The last
// stream also reports the totals. Returns whether the stream's tail is to be copied.
GPK_HD bool emit_one(const Args& a, uint32_t j, uint32_t S, const Tot& t) {
  gpk_tls_stream* e = &a.out.streams[j];
  const Tot end = TotAdd()(t, own_of(a, j));
  if (j == S - 1) {
    uint64_t* c = a.out.counts;
    c[0] = S, c[1] = end.framed, c[2] = end.rec, c[3] = end.failed, c[4] = end.hello;
    c[5] = !fits(a.out, end);
    c[6] = end.rec, c[7] = end.hello, c[8] = end.sni, c[9] = end.tail;
    c[10] = c[11] = 0;
  }
  e->rec0 = t.rec;
  e->hello0 = t.hello;
  e->sni0 = t.sni;
  e->tail_off = t.tail;
  if (!a.framed[j]) return false;
  if (!fits(a.out, end)) {
    e->status |= GPK_TLSS_ST_DROPPED;
    return false;
  }
  View v;
  resolve(a, j, v);
  Framed f;
  frame<true>(v, j, f, a.out.recs + t.rec, a.out.hellos + t.hello, a.out.snis, t.sni);
  return f.tail_len != 0;
}

__global__ void __launch_bounds__(kBlk) size_kernel(const Args a) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < stream_count(a)) size_one(a, (uint32_t)j);
}

__global__ void __launch_bounds__(kBlk) emit_kernel(const Args a, const Tot* starts) {
  const uint32_t S = stream_count(a);
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j < S) emit_one(a, (uint32_t)j, S, starts[j]);
}

bool bad_out(const gpk_tls_stream_out* o) {
  return !o || !o->streams || !o->counts || ((uintptr_t)o->streams & 7) || ((uintptr_t)o->recs & 7) ||
         ((uintptr_t)o->hellos & 7) || (o->rec_cap && !o->recs) || (o->hello_cap && !o->hellos) ||
         (o->sni_cap && !o->snis) || (o->tail_cap && !o->tails);
}

bool bad_args(const gpk_parser* p, const gpk_batch* b, const gpk_results* r, const gpk_tcp_streams* as,
              const gpk_tls_stream_in* in, const gpk_tls_stream_out* o) {
  return bad_out(o) || bad_stream_args<TlsPass>(p, b, r, as, in);
}

}  // namespace

struct gpk_tls_stream_decoder {
  int device = 0;
  uint64_t cap = 0;
  uint64_t* cut = nullptr;      // [cap]
  uint32_t* nostart = nullptr;  // [cap]
  uint32_t* framed = nullptr;   // [cap]
  Tot* starts = nullptr;        // [cap]
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  gpk::Workspace ws;
  void carve() {
    ws.take(cut, cap), ws.take(nostart, cap), ws.take(framed, cap), ws.take(starts, cap);
    ws.take(tmp, tmp_bytes ? tmp_bytes : 4);
  }
};

extern "C" int gpk_tls_stream_decoder_create(gpk_tls_stream_decoder** out, int device, uint64_t max_streams) {
  if (const int rc = gpk::check_create(out, device, max_streams, 1ull << 28)) return rc;
  gpk::DeviceScope dscope(device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  gpk_tls_stream_decoder* h = new (std::nothrow) gpk_tls_stream_decoder();
  if (!h) return GPK_ENOMEM;
  h->device = device;
  h->cap = max_streams;
  const bool ok = hipcub::DeviceScan::ExclusiveScan(nullptr, h->tmp_bytes,
                                                    TotIn(hipcub::CountingInputIterator<uint32_t>(0), TotOf{Args{}}),
                                                    (Tot*)nullptr, TotAdd(), Tot{0, 0, 0, 0, 0, 0},
                                                    (int)max_streams) == hipSuccess;
  h->carve();
  if (!ok || !h->ws.alloc()) {
    delete h;
    return GPK_ENOMEM;
  }
  h->carve();
  *out = h;
  return GPK_OK;
}

extern "C" int gpk_tls_stream_decoder_destroy(gpk_tls_stream_decoder* d) {
  if (!d) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  (void)hipDeviceSynchronize();
  d->ws.release();
  delete d;
  return GPK_OK;
}

namespace {

struct Launch {
  gpk_tls_stream_decoder* h;
  Args a;
  hipStream_t s;
};

int launch_step(const gpk::DevTables* tab, void* arg) {
  Launch& l = *static_cast<Launch*>(arg);
  gpk_tls_stream_decoder* h = l.h;
  Args& a = l.a;
  hipStream_t s = l.s;
  a.tab = tab;
  const unsigned blocks = (unsigned)((a.n + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(init_kernel<TlsPass>, dim3(blocks), dim3(kBlk), 0, s, a);
  if (a.as.chunk_cap) {
    const uint64_t cb = (a.as.chunk_cap + kBlk - 1) / kBlk;
    if (cb >= (1ull << 31)) return GPK_EINVAL;
    hipLaunchKernelGGL(cut_kernel<TlsPass>, dim3((unsigned)cb), dim3(kBlk), 0, s, a);
  }
  hipLaunchKernelGGL(size_kernel, dim3(blocks), dim3(kBlk), 0, s, a);
  size_t tb = h->tmp_bytes;
  const TotIn in(hipcub::CountingInputIterator<uint32_t>(0), TotOf{a});
  if (hipcub::DeviceScan::ExclusiveScan(h->tmp, tb, in, h->starts, TotAdd(), Tot{0, 0, 0, 0, 0, 0}, (int)a.n, s) !=
      hipSuccess)
    return GPK_EHIP;
  hipLaunchKernelGGL(emit_kernel, dim3(blocks), dim3(kBlk), 0, s, a, (const Tot*)h->starts);
  if (a.out.tail_cap) hipLaunchKernelGGL(tail_kernel<TlsPass>, dim3(blocks), dim3(kBlk), 0, s, a);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

}  // namespace

extern "C" int gpk_tls_streams(gpk_tls_stream_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* b,
                               const gpk_results* r, const gpk_tcp_streams* as, const gpk_tls_stream_in* in,
                               const gpk_tls_stream_out* o, void* stream) {
  if (!d || !ctx || bad_args(parser, b, r, as, in, o) || b->n > d->cap) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(o->counts, 0, 12 * 8, s) != hipSuccess) return GPK_EHIP;
  if (b->n == 0) return GPK_OK;
  Launch l{d, make_args<TlsPass>(b, r, as, in, o), s};
  l.a.cut = d->cut, l.a.nostart = d->nostart, l.a.framed = d->framed;
  return gpk_with_device_tables(ctx, parser, stream, launch_step, &l);
}

extern "C" int gpk_tls_streams_host(const gpk_parser* parser, const gpk_batch* b, const gpk_results* r,
                                    const gpk_tcp_streams* as, const gpk_tls_stream_in* in,
                                    const gpk_tls_stream_out* o) {
  if (bad_args(parser, b, r, as, in, o)) return GPK_EINVAL;
  for (int k = 0; k < 12; k++) o->counts[k] = 0;
  if (b->n == 0) return GPK_OK;
  Args a = make_args<TlsPass>(b, r, as, in, o);
  a.tab = gpk_parser_tables(parser);
  const uint32_t S = stream_count(a);
  if (S == 0) return GPK_OK;
  a.cut = new (std::nothrow) uint64_t[S];
  a.nostart = new (std::nothrow) uint32_t[S];
  a.framed = new (std::nothrow) uint32_t[S];
  int rc = GPK_ENOMEM;
  if (a.cut && a.nostart && a.framed) {
    host_cut(a, S);
    for (uint32_t j = 0; j < S; j++) size_one(a, j);
    Tot t{0, 0, 0, 0, 0, 0};
    for (uint32_t j = 0; j < S; j++) {
      const Tot own = own_of(a, j);
      if (emit_one(a, j, S, t)) host_tail(a, j, t.tail);
      t = TotAdd()(t, own);
    }
    rc = GPK_OK;
  }
  delete[] a.cut;
  delete[] a.nostart;
  delete[] a.framed;
  return rc;
}
