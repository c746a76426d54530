// gpk_streams.h — what the passes over reassembled TCP streams share
// (gpk_tls_streams.hip, gpk_dns_streams.hip; library-internal, in the spirit of
// gpk_postpass.h): the part of a stream pass that does not know the protocol.
//
//   StreamArgs<P> the call: the batch, the assembler's outputs, what the streams
//                 carry in, the outputs, and the per-stream workspace
//   View/resolve  a stream's logical buffer (carried tail, then the new bytes in
//                 front of the cut) and its state before framing: carried final
//                 states, the candidate rule, no start, too big, bad tail
//   init_kernel   one lane per possible stream: no cut, no Skip == -1 seen
//   cut_kernel    one lane per chunk: an atomicMin per stream of the position of
//                 the first chunk with Skip > 0 (where the logical buffer is
//                 cut), and a flag for a chunk with Skip == -1. No lane scans its
//                 stream's chunk table.
//   host_cut      the two on host arrays
//   tail_parts    where a stream's unfinished tail lies in its two buffers
//   tail_kernel   a wave looks at 64 streams, one per lane, and moves the tail of
//                 each that has one with all its lanes (copy_bytes of gpk_copy.h)
//
// A pass P names its ABI: the structs In (state, tail_off, tail_len, tails, n,
// tail_bytes, flags), Out (streams, tails) and Stream (state, status, tail_in,
// consumed, tail_len, tail_off), and the constants kLayer (the candidate's
// layer type), kNew, kSynced, kNone, kNostart, kNState, kFrameUnstarted,
// kAllFlags, kDropped, kTooBig, kBadTail.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/gpk_tcpasm.h"
#include "gpk_copy.h"
#include "gpk_tunnel_rules.h"

namespace {  // no device symbol is exported

constexpr int kBlk = 256;
constexpr int kSlotTcp = 5;  // gpk_layout slot of TCP
constexpr uint64_t kNoCut = ~0ull;

template <typename P>
struct StreamArgs {
  const uint8_t* data;  // the batch
  const uint64_t* offsets;
  const gpk_layout* layouts;
  const gpk::DevTables* tab;
  uint64_t n;  // the batch's packets: no more streams exist
  gpk_tcp_streams as;
  typename P::In in;
  typename P::Out out;
  uint64_t* cut;      // [n] offset of the first Skip > 0 inside the stream's bytes, or kNoCut
  uint32_t* nostart;  // [n] 1: a chunk with Skip == -1
  uint32_t* framed;   // [n] 1: the stream was framed in this call
};

template <typename P>
GPK_HD uint32_t stream_count(const StreamArgs<P>& a) {
  const uint64_t s = a.as.counts[0];
  return (uint32_t)(s < a.n ? s : a.n);
}

// A stream's logical buffer and what the call knows about it
struct View {
  const uint8_t* tail;  // tail_in bytes
  const uint8_t* nb;    // the new bytes
  uint32_t tail_in, len;  // len: tail_in + the new bytes in front of the cut
  uint32_t state, status;
  bool frame, lost, closed;
};

// TCP.NextLayerType() of the stream's creating packet (tcp.go:591-597)
template <typename P>
GPK_HD bool candidate(const StreamArgs<P>& a, uint32_t j) {
  const uint32_t p = a.as.stream_first[j];
  if (p >= a.n) return false;
  const uint32_t s = a.layouts[p].start[kSlotTcp], e = a.layouts[p].end[kSlotTcp];
  if (s == GPK_LAYOUT_ABSENT || e < s || e - s < 20) return false;
  return gpk::tun::port_type(a.tab->tcp_port, a.data + a.offsets[p] + s) == P::kLayer;
}

template <typename P>
GPK_HD void resolve(const StreamArgs<P>& a, uint32_t j, View& v) {
  v.tail = v.nb = nullptr;
  v.tail_in = v.len = v.status = 0;
  v.frame = v.lost = v.closed = false;
  const uint32_t st = j < a.in.n ? a.in.state[j] : (uint32_t)P::kNew;
  if (st != P::kNew && st != P::kSynced) {  // final: kept
    v.state = st < P::kNState ? st : (uint32_t)P::kNone;
    return;
  }
  if (st == P::kNew && !candidate(a, j)) {
    v.state = P::kNone;
    return;
  }
  if (a.nostart[j] && !(a.in.flags & P::kFrameUnstarted)) {
    v.state = P::kNostart;
    return;
  }
  v.frame = true;
  v.state = P::kSynced;
  v.closed = a.as.stream_closed[j] != GPK_TCPASM_OPEN;
  uint64_t tl = 0, to = 0;
  if (st == P::kSynced) {
    tl = a.in.tail_len[j];
    to = a.in.tail_off[j];
    if (tl && (to > a.in.tail_bytes || tl > a.in.tail_bytes - to)) v.status = P::kBadTail;
  }
  const uint64_t d0 = a.as.stream_data0[j], d1 = a.as.stream_data0[j + 1];
  uint64_t nbytes = d1 >= d0 ? d1 - d0 : 0;
  const uint64_t c = a.cut[j];
  v.lost = c != kNoCut;
  if (v.lost && c < nbytes) nbytes = c;
  if (d1 < d0 || d1 > a.as.data_cap || tl + nbytes >= (1ull << 32)) v.status |= P::kTooBig;
  if (v.status) {  // as a loss, and no byte is read
    v.lost = true;
    return;
  }
  v.tail = a.in.tails + to;
  v.nb = a.as.data + d0;
  v.tail_in = (uint32_t)tl;
  v.len = (uint32_t)(tl + nbytes);
}

// where the tail of stream j lies: [consumed, tail_in) of the carried tail (n0 bytes at s0), then the new bytes
// from max(consumed, tail_in) on (n1 bytes at s1)
template <typename P>
GPK_HD void tail_parts(const StreamArgs<P>& a, uint32_t j, const uint8_t*& s0, uint32_t& n0, const uint8_t*& s1,
                       uint32_t& n1) {
  const typename P::Stream& e = a.out.streams[j];
  n0 = e.consumed < e.tail_in ? e.tail_in - e.consumed : 0;
  n1 = e.tail_len - n0;
  s0 = n0 ? a.in.tails + a.in.tail_off[j] + e.consumed : nullptr;  // tail_in > 0: j < in.n
  s1 = n1 ? a.as.data + a.as.stream_data0[j] + (e.consumed + n0 - e.tail_in) : nullptr;
}

template <typename P>
__global__ void __launch_bounds__(kBlk) init_kernel(const StreamArgs<P> a) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (j >= a.n) return;
  a.cut[j] = kNoCut;
  a.nostart[j] = 0;
  a.framed[j] = 0;
}

template <typename P>
__global__ void __launch_bounds__(kBlk) cut_kernel(const StreamArgs<P> a) {
  const uint64_t have = a.as.counts[1] < a.as.chunk_cap ? a.as.counts[1] : a.as.chunk_cap;
  const uint64_t c = (uint64_t)blockIdx.x * kBlk + threadIdx.x;
  if (c >= have) return;
  const int64_t skip = a.as.chunks[c].skip;
  if (skip == 0) return;
  const uint32_t j = a.as.chunks[c].stream;
  if (j >= stream_count(a)) return;
  if (skip < 0) {
    a.nostart[j] = 1;
  } else {
    const uint64_t d0 = a.as.stream_data0[j], at = a.as.chunks[c].dst;
    atomicMin((unsigned long long*)&a.cut[j], (unsigned long long)(at >= d0 ? at - d0 : 0));
  }
}

// init_kernel and cut_kernel over host arrays of S streams
template <typename P>
void host_cut(const StreamArgs<P>& a, uint32_t S) {
  for (uint32_t j = 0; j < S; j++) a.cut[j] = kNoCut, a.nostart[j] = 0, a.framed[j] = 0;
  const uint64_t have = a.as.counts[1] < a.as.chunk_cap ? a.as.counts[1] : a.as.chunk_cap;
  for (uint64_t c = 0; c < have; c++) {
    const gpk_tcp_chunk& ch = a.as.chunks[c];
    if (ch.skip == 0 || ch.stream >= S) continue;
    if (ch.skip < 0) {
      a.nostart[ch.stream] = 1;
    } else {
      const uint64_t d0 = a.as.stream_data0[ch.stream], at = ch.dst >= d0 ? ch.dst - d0 : 0;
      if (at < a.cut[ch.stream]) a.cut[ch.stream] = at;
    }
  }
}

template <typename P>
__global__ void __launch_bounds__(kBlk) tail_kernel(const StreamArgs<P> a) {
  const uint32_t S = stream_count(a);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t base = ((uint64_t)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6)) * 64;
  if (base >= S) return;
  const uint64_t j = base + lane;
  bool has = false;
  if (j < S) {
    const typename P::Stream& e = a.out.streams[j];
    has = e.state == P::kSynced && e.tail_len && !(e.status & P::kDropped);
  }
  for (uint64_t todo = __ballot(has); todo; todo &= todo - 1) {  // wave-uniform
    const uint32_t k = (uint32_t)(base + __builtin_ctzll(todo));
    const uint8_t *s0, *s1;
    uint32_t n0, n1;
    tail_parts(a, k, s0, n0, s1, n1);
    uint8_t* dst = a.out.tails + a.out.streams[k].tail_off;
    if (n0) gpk::copy_bytes(dst, s0, n0, lane);
    if (n1) gpk::copy_bytes(dst + n0, s1, n1, lane);
  }
}

// the tail of stream j on host arrays, to tails + at
template <typename P>
void host_tail(const StreamArgs<P>& a, uint32_t j, uint64_t at) {
  const uint8_t *s0, *s1;
  uint32_t n0, n1;
  tail_parts(a, j, s0, n0, s1, n1);
  if (n0) memcpy(a.out.tails + at, s0, n0);
  if (n1) memcpy(a.out.tails + at + n0, s1, n1);
}

// the argument faults of both entries that do not concern the outputs
template <typename P>
bool bad_stream_args(const gpk_parser* p, const gpk_batch* b, const gpk_results* r, const gpk_tcp_streams* as,
                     const typename P::In* in) {
  if (!p || !b || !r || !as || !as->counts) return true;
  if (b->n >= (1ull << 32)) return true;
  if (b->n && (!b->data || !b->offsets || !r->layouts || !as->chunks || !as->stream_first || !as->stream_closed ||
               !as->stream_data0 || !as->data))
    return true;
  if (in) {
    if ((in->flags & ~P::kAllFlags) || in->n > b->n) return true;
    if (in->n && (!in->state || !in->tail_off || !in->tail_len)) return true;
    if (in->tail_bytes && !in->tails) return true;
  }
  return false;
}

template <typename P>
StreamArgs<P> make_args(const gpk_batch* b, const gpk_results* r, const gpk_tcp_streams* as, const typename P::In* in,
                  const typename P::Out* o) {
  StreamArgs<P> a{};
  a.data = b->data;
  a.offsets = b->offsets;
  a.layouts = r->layouts;
  a.n = b->n;
  a.as = *as;
  if (in) a.in = *in;
  a.out = *o;
  return a;
}

}  // namespace
