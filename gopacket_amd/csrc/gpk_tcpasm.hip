// gpk_tcpasm.hip — TCP stream reassembly of a decoded, connection-grouped batch
// (include/gpk_tcpasm.h): tcpassembly's AssembleWithTimestamp / insertIntoConn /
// addNextFromConn / sendToConnection and FlushAll for every key of a batch,
// then the byte movement.
//
//   1. prep_kernel    one lane per packet: Seq, payload length, payload start,
//                     SYN / FIN|RST and the carried code, once, in 16 bytes
//   2. hipcub scan    page counts in group order: every key's slice of the page
//                     and chunk workspaces (a packet makes max(1, ceil(len/1900))
//                     pages or one direct chunk, never both, so the slice can
//                     hold both the key's page list and its chunks)
//   3. plan_kernel    one wave per key, its packets in batch order. While the
//                     key's list is empty and nextSeq valid, a wave prefix sum
//                     of payload lengths and a ballot retire the in-order run at
//                     the head of the 64 packets in hand in one step. Otherwise
//                     one packet per step: the back-scan of traverseConn looks
//                     at 64 list entries per ballot, an insert shifts the tail
//                     in parallel, pops advance a head index that returns to 0
//                     when the list empties. The first 256 list positions are
//                     in LDS: the whole list for keys of up to 256 pages (one
//                     instantiation), and for the others whatever lies beyond
//                     is in the key's slice of the page workspace. Chunks go to the key's
//                     slice of the chunk workspace in delivery order, which is
//                     stream-major inside a key. With time (a template parameter
//                     beside SMALL: the untimed instantiations compile from the
//                     code they always had) the key also keeps lastSeen, the
//                     maximum of its calls' timestamps. Nothing reads it before
//                     the end of the batch, so every lane keeps the maximum of
//                     the calls it held (one compare per step, off the chain
//                     that carries nextSeq) and one wave maximum per key joins
//                     them at the end; a new connection resets all lanes. A wave
//                     maximum per in-order run cost 0.5 us per 64-packet step.
//                     FlushWithOptions{T} runs where FlushAll does, with the
//                     same pop / send / close.
//   4. hipcub scans   stream numbers, chunk bases, byte bases (by creating
//                     packet), pending bases (by group)
//   5. finish_kernel  per-stream and per-group arrays, stream_of, counts
//      pend_kernel    the pages still listed, by group
//   6. emit_kernel    one wave per chunk: its record goes to its stream-major
//                     place, its bytes move with destination-aligned 16-byte
//                     stores, the source realigned in registers (copy_bytes of
//                     gpk_copy.h).
// Every state variable of a key is computed identically by all 64 lanes from
// shuffled or broadcast values, so the control flow around ballots, shuffles
// and barriers is wave-uniform; blocks of the plan kernel are one wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>

#include "../../include/gpk_tcpasm.h"
#include "gpk_copy.h"
#include "gpk_scan.h"
#include "gpk_workspace.h"

namespace {

constexpr int kSlotTcp = 5;  // gpk_layout slot of TCP
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kSmallCap = 256;
constexpr uint32_t kPage = GPK_TCPASM_PAGE_BYTES;
constexpr int64_t kU32 = 1ll << 32;
constexpr uint32_t kSyn = 1, kEnd = 2, kCarryConn = 4, kCarryPage = 8;  // info.w; page number << 16
constexpr uint32_t kMetaEnd = 1u << 31;                                 // list meta: page | len << 16 | End << 31

struct Work {
  uint4* info;          // [n]   x = Seq, y = len(payload), z = payload start in the packet, w = flags
  uint32_t* creator;    // [n]   the packet that created the stream this packet was routed to, or kNone
  uint32_t* s_made;     // [n]   by creating packet: 1 if it created a stream instance
  uint32_t* s_nchunks;  // [n]     its chunks
  uint64_t* s_nbytes;   // [n]     its bytes
  uint32_t* s_wk0;      // [n]     its first slot in the chunk workspace
  uint32_t* s_closed;   // [n]     its closing call code
  uint32_t* s_group;    // [n]
  uint32_t* snum;       // [n]   scans by creating packet
  uint32_t* cbase;      // [n]
  uint64_t* dbase;      // [n]
  uint32_t* g_creator;  // [n]   by group: the open connection's creating packet, or kNone
  uint32_t* g_npend;    // [n]     pages still listed
  uint32_t* g_head;     // [n]     where they start inside the key's slice
  uint32_t* pbase;      // [n]   scan of g_npend
  uint32_t* wbase;      // [n+1] scan: slice bounds in group (perm) order
  gpk_tcp_chunk* wc;    // [wcap] chunk workspace; stream = creating packet, dst = offset inside the stream
  uint32_t* pg_seq;     // [wcap] page workspace
  uint32_t* pg_pkt;     // [wcap]
  uint32_t* pg_meta;    // [wcap]
  uint64_t wcap;
};

__host__ __device__ __forceinline__ uint32_t page_count(uint32_t plen, uint32_t fw) {
  if (fw & (kCarryConn | kCarryPage)) return 1;
  return plen ? (plen + kPage - 1) / kPage : 1;
}

__global__ void __launch_bounds__(256) prep_kernel(const uint8_t* data, const uint64_t* offsets,
                                                   const gpk_layout* layouts, const int32_t* group_of, uint64_t n,
                                                   uint64_t carried, const uint32_t* carry_code, Work w) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w.creator[i] = kNone;
  w.s_made[i] = 0;
  w.s_nchunks[i] = 0;
  w.s_nbytes[i] = 0;
  w.g_npend[i] = 0;
  w.g_creator[i] = kNone;
  uint4 inf = make_uint4(0, 0, 0, 0);
  if (group_of[i] >= 0) {  // keyed: the TCP slot holds a successful decode of >= 20 bytes
    const uint32_t t0 = layouts[i].start[kSlotTcp], tlen = layouts[i].end[kSlotTcp] - t0;
    const uint8_t* t = data + offsets[i] + t0;
    uint32_t hdr = (uint32_t)(t[12] >> 4) * 4;
    if (hdr > tlen) hdr = tlen;
    const uint32_t seq = (uint32_t)t[4] << 24 | (uint32_t)t[5] << 16 | (uint32_t)t[6] << 8 | t[7];
    uint32_t fw = ((t[13] & 2u) ? kSyn : 0u) | ((t[13] & 5u) ? kEnd : 0u);
    if (i < carried) {
      const uint32_t c = carry_code[i];
      fw |= ((c & GPK_TCPASM_CARRY_CONN) ? kCarryConn : 0u) | ((c & GPK_TCPASM_CARRY_PAGE) ? kCarryPage : 0u) |
            (c & 0xFFFFu) << 16;
      if (!(fw & (kCarryConn | kCarryPage))) fw |= kCarryConn | kCarryPage;  // neither: a bad entry
    }
    inf = make_uint4(seq, tlen - hdr, t0 + hdr, fw);
  }
  w.info[i] = inf;
}

// Sequence.Difference (assembly.go:57-64)
__device__ __forceinline__ int64_t seq_diff(int64_t s, int64_t t) {
  if (s > kU32 - kU32 / 4 && t < kU32 / 4)
    t += kU32;
  else if (t > kU32 - kU32 / 4 && s < kU32 / 4)
    s += kU32;
  return t - s;
}

struct PlanArgs {
  const uint32_t* perm;
  const uint32_t* start;
  const uint32_t* gcounts;
  const int64_t* carry_seq;
  uint32_t max_pages, flush;
  int32_t* verdict;
  int64_t* conn_seq;
  Work w;
  gpk_tcpasm_time tm;  // read by the timed instantiations only
};

// The first kSmallCap positions of the list of the key a block (one wave) works on.
// At file scope so that every access is compiled as an LDS access.
// (One spare slot takes the LDS half of a store that goes to the slice: an LDS and
// a global access are never two arms of one branch, which the compiler would
// merge into a single access through a generic pointer.)
__shared__ uint32_t s_seq[kSmallCap + 1], s_pkt[kSmallCap + 1], s_meta[kSmallCap + 1];

// One key's assembler state, identical in all 64 lanes.
template <bool SMALL>
struct Key {
  // the page list: entries [head, head + len) of the key's slice; its first
  // kSmallCap positions are in LDS (s_seq, s_pkt, s_meta), the others (large keys only) in the slice
  uint32_t *gseq, *gpkt, *gmeta;  // the key's slice of the page workspace
  gpk_tcp_chunk* wc;              // the key's chunk slice
  uint32_t lane, g, w0;
  uint32_t head = 0, len = 0, used = 0;
  bool open = false;
  int64_t next = -1;
  uint32_t cr = kNone, schunks = 0, swk0 = 0;
  uint64_t sbytes = 0;
  uint32_t nret = 0;
  bool last_end = false;
  const Work& w;

  __device__ Key(const Work& w_) : w(w_) {}

  __device__ uint32_t ld(const uint32_t* lds, const uint32_t* glob, uint32_t e) const {
    if constexpr (SMALL) return lds[e];
    const bool in = e < (uint32_t)kSmallCap;
    uint32_t v = lds[in ? e : (uint32_t)kSmallCap];
    asm volatile("" : "+v"(v));  // the same for loads: the LDS value is settled before the other arm
    if (!in) v = glob[e];
    return v;
  }
  __device__ void st(uint32_t* lds, uint32_t* glob, uint32_t e, uint32_t v) {
    if constexpr (SMALL) {
      lds[e] = v;
    } else {
      const bool in = e < (uint32_t)kSmallCap;
      lds[in ? e : (uint32_t)kSmallCap] = v;
      if (!in) glob[e] = v;
    }
  }

  // Order list writes before the reads of other lanes. A block is one wave, so
  // for LDS an LDS-only fence does (a full barrier would also wait for the chunk
  // records still on their way to memory). The slice part of a large key's list
  // is global memory: there the full barrier stays.
  __device__ void list_sync(uint32_t top) {
    if (!SMALL && top > (uint32_t)kSmallCap) {
      __syncthreads();
      return;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
  }

  __device__ void open_conn(uint32_t pkt, int64_t seq) {
    open = true;
    next = seq;
    cr = pkt;
    sbytes = 0;
    schunks = 0;
    swk0 = used;
  }

  __device__ void emit(uint32_t src, uint32_t off, uint32_t ln, int64_t skip, uint32_t call, uint32_t flags) {
    if (lane == 0) {
      gpk_tcp_chunk c;
      c.dst = sbytes;
      c.skip = skip;
      c.src = src;
      c.src_off = off;
      c.len = ln;
      c.call = call;
      c.stream = cr;
      c.flags = flags;
      wc[used] = c;
    }
    used++;
    schunks++;
    sbytes += ln;
    nret++;
    last_end = (flags & GPK_TCP_END) != 0;
  }

  // byteSpan (:612-623) on (off, ln) of the source payload; moves next
  __device__ void byte_span(int64_t received, uint32_t& off, uint32_t& ln) {
    if (next != -1) {
      const int64_t span = seq_diff(received, next);
      if (span > 0) {
        if ((int64_t)ln < span) {
          off += ln;
          ln = 0;
          return;  // (nil, expected)
        }
        off += (uint32_t)span;
        ln -= (uint32_t)span;
        next = (next + ln) & (kU32 - 1);
        return;
      }
    }
    next = (received + ln) & (kU32 - 1);
  }

  // addNextFromConn (:763-783)
  __device__ void pop(uint32_t call) {
    const int64_t es = ld(s_seq, gseq, head);
    const uint32_t ep = ld(s_pkt, gpkt, head), em = ld(s_meta, gmeta, head);
    int64_t skip = 0;
    if (next == -1) {
      skip = -1;
    } else {
      const int64_t d = seq_diff(next, es);
      if (d > 0) skip = d;
    }
    uint32_t off = (em & 0xFFFFu) * kPage, ln = (em >> 16) & 0x7FFFu;
    byte_span(es, off, ln);
    emit(ep, off, ln, skip, call, (em & kMetaEnd) ? GPK_TCP_END : 0u);
    head++;
    len--;
    if (!len) head = 0;  // an empty list starts again at the LDS end of the slice
  }

  // addContiguous (:639-643) and the tail of sendToConnection (:633-635)
  __device__ void send(uint32_t call) {
    while (len && seq_diff(next, (int64_t)ld(s_seq, gseq, head)) <= 0) pop(call);
    if (last_end) close(call);
  }

  __device__ void end_stream(uint32_t code) {
    if (lane == 0) {
      w.s_made[cr] = 1;
      w.s_nchunks[cr] = schunks;
      w.s_nbytes[cr] = sbytes;
      w.s_wk0[cr] = w0 + swk0;
      w.s_closed[cr] = code;
      w.s_group[cr] = g;
    }
  }

  // closeConnection (:669-679): the remaining pages are dropped
  __device__ void close(uint32_t call) {
    end_stream(call);
    head = 0;
    len = 0;
    open = false;
    next = -1;
  }

  __device__ void put_page(uint32_t at, uint32_t seq, uint32_t pkt, uint32_t plen, uint32_t k, uint32_t pages,
                           bool end) {
    const uint32_t ln = plen - k * kPage < kPage ? plen - k * kPage : kPage;
    st(s_seq, gseq, at, seq + k * kPage);
    st(s_pkt, gpkt, at, pkt);
    st(s_meta, gmeta, at, k | ln << 16 | ((end && k + 1 == pages) ? kMetaEnd : 0u));
  }

  // pagesFromTCP, traverseConn, pushBetween (:686-759)
  __device__ void insert(uint32_t seq, uint32_t pkt, uint32_t plen, bool end) {
    const uint32_t pages = plen ? (plen + kPage - 1) / kPage : 1;
    uint32_t pos = 0;
    for (uint32_t hi = len; hi > 0;) {  // from the back: the first entry not before seq
      const uint32_t lo = hi > 64 ? hi - 64 : 0;
      const uint32_t e = lo + lane;
      const bool val = e < hi;
      const int64_t es = val ? ld(s_seq, gseq, head + e) : 0;
      const uint64_t m = __ballot(val && seq_diff(es, (int64_t)seq) >= 0);
      if (m) {
        pos = lo + 64 - (uint32_t)__builtin_clzll(m);
        break;
      }
      hi = lo;
    }
    for (uint32_t hi = len; hi > pos;) {  // move [pos, len) up by `pages`, from the tail
      const uint32_t lo = hi - pos > 64 ? hi - 64 : pos;
      const uint32_t e = head + lo + lane;
      const bool val = lo + lane < hi;
      const uint32_t a = val ? ld(s_seq, gseq, e) : 0, b = val ? ld(s_pkt, gpkt, e) : 0, c = val ? ld(s_meta, gmeta, e) : 0;
      list_sync(head + len + pages);
      if (val) {
        st(s_seq, gseq, e + pages, a);
        st(s_pkt, gpkt, e + pages, b);
        st(s_meta, gmeta, e + pages, c);
      }
      list_sync(head + len + pages);
      hi = lo;
    }
    for (uint32_t k = lane; k < pages; k += 64) put_page(head + pos + k, seq, pkt, plen, k, pages, end);
    len += pages;
    list_sync(head + len);
  }
};

// max over the wave of v (lanes that do not take part pass INT64_MIN)
__device__ __forceinline__ int64_t wave_max(int64_t v) {
  for (int m = 32; m; m >>= 1) {
    const int64_t o = (int64_t)__shfl_xor((long long)v, m);
    if (o > v) v = o;
  }
  return v;
}

template <bool SMALL, bool TIMED>
__global__ void __launch_bounds__(64) plan_kernel(PlanArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint32_t G = a.gcounts[0], K = a.gcounts[1];
  if (a.w.wbase[K] > a.w.wcap) return;  // see finish_kernel
  for (uint32_t g = blockIdx.x; g < G; g += gridDim.x) {
    const uint32_t s = a.start[g], k = a.start[g + 1] - s;
    const uint32_t w0 = a.w.wbase[s], cap = a.w.wbase[s + k] - w0;
    if ((cap <= (uint32_t)kSmallCap) != SMALL) continue;
    Key<SMALL> c(a.w);
    c.lane = lane;
    c.g = g;
    c.w0 = w0;
    c.wc = a.w.wc + w0;
    c.gseq = a.w.pg_seq + w0;
    c.gpkt = a.w.pg_pkt + w0;
    c.gmeta = a.w.pg_meta + w0;
    // the packets of the next step are fetched while this one runs: info one step
    // ahead, the index it hangs on two steps ahead
    uint32_t pkt_a = 0, pkt_b = 0;
    uint4 inf_a = make_uint4(0, 0, 0, 0);
    // TIMED: this lane's share of conn.lastSeen (the maximum over the calls it held), and seen[] one step
    // ahead like info
    int64_t lane_seen = INT64_MIN, sn_a = INT64_MIN;
    if (lane < k) {
      pkt_a = a.perm[s + lane];
      inf_a = a.w.info[pkt_a];
      if constexpr (TIMED) sn_a = a.tm.seen[pkt_a];
    }
    if (64 + lane < k) pkt_b = a.perm[s + 64 + lane];
    for (uint32_t c0 = 0; c0 < k; c0 += 64) {
      const uint32_t cnt = k - c0 < 64 ? k - c0 : 64;
      const uint32_t pkt = pkt_a;
      const uint4 inf = inf_a;
      const int64_t sn = sn_a;
      pkt_a = pkt_b;
      inf_a = make_uint4(0, 0, 0, 0);
      sn_a = INT64_MIN;
      if (c0 + 64 + lane < k) {
        inf_a = a.w.info[pkt_a];
        if constexpr (TIMED) sn_a = a.tm.seen[pkt_a];
      }
      pkt_b = 0;
      if (c0 + 128 + lane < k) pkt_b = a.perm[s + c0 + 128 + lane];
      int32_t my_v = 0;
      uint32_t my_cr = kNone;
      for (uint32_t t = 0; t < cnt;) {
        // ---- the in-order run at the head of [t, cnt): no flags, seq == nextSeq + the lengths before it
        if (c.open && c.next != -1 && c.len == 0) {
          const bool in = lane >= t && lane < cnt;
          uint32_t inc = in ? inf.y : 0;  // inclusive prefix sum of the lengths, mod 2^32
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
            if ((int)lane >= d) inc += up;
          }
          const uint32_t before = inc - (in ? inf.y : 0);
          // (lengths below 2^25: the 64 of a step sum below 2^32, so the scan is exact)
          const bool ok = in && inf.w == 0 && inf.y < (1u << 25) && inf.x == (uint32_t)c.next + before;
          uint64_t stop = __ballot(in && !ok);
          if (cnt < 64) stop |= ~0ull << cnt;
          const uint32_t first = stop ? (uint32_t)__builtin_ctzll(stop) : 64u;
          const uint32_t run = first - t;
          if (run) {
            if (lane >= t && lane < first) {
              gpk_tcp_chunk ch;
              ch.dst = c.sbytes + before;
              ch.skip = 0;
              ch.src = pkt;
              ch.src_off = 0;
              ch.len = inf.y;
              ch.call = pkt;
              ch.stream = c.cr;
              ch.flags = 0;
              c.wc[c.used + (lane - t)] = ch;
              my_v = GPK_TCPASM_DIRECT;
              my_cr = c.cr;
            }
            // the bytes of the run: the scan at its last lane (lanes before t added nothing)
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, (int)(first - 1));
            c.sbytes += total;
            c.next = ((int64_t)(uint32_t)((uint32_t)c.next + total));
            c.schunks += run;
            c.used += run;
            if constexpr (TIMED) {  // every call of the run: if lastSeen.Before(ts) lastSeen = ts (:567-569)
              if (lane >= t && lane < first && lane_seen < sn) lane_seen = sn;
            }
            t = first;
            continue;
          }
        }
        // ---- one packet (assembly.go:536-610)
        const uint32_t seq = (uint32_t)__builtin_amdgcn_readlane((int)inf.x, (int)t);
        const uint32_t plen = (uint32_t)__builtin_amdgcn_readlane((int)inf.y, (int)t);
        const uint32_t fw = (uint32_t)__builtin_amdgcn_readlane((int)inf.w, (int)t);
        const uint32_t tp = (uint32_t)__builtin_amdgcn_readlane((int)pkt, (int)t);
        const bool syn = fw & kSyn, end = fw & kEnd;
        int32_t v;
        uint32_t cr_t = kNone;
        c.nret = 0;
        c.last_end = false;
        if (fw & (kCarryConn | kCarryPage)) {  // a carried entry: no Assemble call
          const uint32_t pg = fw >> 16, pages = plen ? (plen + kPage - 1) / kPage : 1;
          v = GPK_TCPASM_EBADCARRY;
          if ((fw & kCarryConn) && !(fw & kCarryPage) && !c.open) {
            c.open_conn(tp, a.carry_seq[tp]);
            if constexpr (TIMED) lane_seen = a.tm.seen[tp];  // the carried connection's lastSeen
            v = GPK_TCPASM_CARRIED;
          } else if ((fw & kCarryPage) && !(fw & kCarryConn) && c.open && pg < pages) {
            if (lane == 0) c.put_page(c.head + c.len, seq, tp, plen, pg, pages, end);
            c.len++;
            c.list_sync(c.head + c.len);
            v = GPK_TCPASM_CARRIED;
          }
          if (v == GPK_TCPASM_CARRIED) cr_t = c.cr;
        } else if (!c.open && !syn && plen == 0) {  // getConnection(key, end = true) (:552-560)
          v = GPK_TCPASM_NOCONN;
        } else {
          if (!c.open) {
            c.open_conn(tp, -1);
            if constexpr (TIMED) lane_seen = INT64_MIN;  // a new connection starts fresh (include/gpk_tcpasm.h)
          }
          if constexpr (TIMED) {  // :567-569
            if (lane == t && lane_seen < sn) lane_seen = sn;
          }
          cr_t = c.cr;
          bool direct = true;
          if (c.next == -1) {
            if (syn) {  // :572-582
              c.emit(tp, 0, plen, 0, tp, GPK_TCP_START);
              c.next = ((int64_t)seq + plen + 1) & (kU32 - 1);
            } else {
              direct = false;
            }
          } else if (seq_diff(c.next, (int64_t)seq) > 0) {  // :589-593
            direct = false;
          } else {  // :594-605
            uint32_t off = 0, ln = plen;
            c.byte_span((int64_t)seq, off, ln);
            c.emit(tp, off, ln, 0, tp, end ? GPK_TCP_END : 0u);
          }
          v = direct ? GPK_TCPASM_DIRECT : GPK_TCPASM_QUEUED;
          if (!direct) {
            if (c.len && (int64_t)c.ld(s_seq, c.gseq, c.head) == c.next) {  // panic("wtf") (:716-718)
              v = GPK_TCPASM_EPANIC;
            } else {
              c.insert(seq, tp, plen, end);
              if (a.max_pages > 0 && c.len >= a.max_pages) c.pop(tp);  // :723-729
            }
          }
          if (c.nret) c.send(tp);  // :606-608
        }
        if (lane == t) {
          my_v = v;
          my_cr = cr_t;
        }
        t++;
      }
      if (lane < cnt) {
        a.verdict[pkt] = my_v;
        a.w.creator[pkt] = my_cr;
      }
    }
    if (a.flush) {  // FlushAll (:279-290): skipFlush (:648-660) until closed
      for (uint32_t r = 0; c.open; r++) {
        const uint32_t call = GPK_TCPASM_CALL_FLUSH | r;
        if (!c.len) {
          c.close(call);
          break;
        }
        c.nret = 0;
        c.last_end = false;
        c.pop(call);
        c.send(call);
      }
    }
    if constexpr (TIMED) {
      const int64_t last_seen = wave_max(lane_seen);
      if (a.tm.flush_older) {  // FlushWithOptions{T, CloseAll} (:238-269) on this connection
        bool flushed = false, closed = false;
        uint32_t r = 0;
        // only the FIRST page's Seen is tested; what is contiguous behind it goes out whatever its age
        while (c.open && c.len && a.tm.seen[c.ld(s_pkt, c.gpkt, c.head)] < a.tm.t) {
          const uint32_t call = GPK_TCPASM_CALL_FLUSH | r++;
          c.nret = 0;
          c.last_end = false;
          c.pop(call);   // skipFlush (:648-660)
          c.send(call);
          flushed = true;
          if (!c.open) closed = true;
        }
        if (a.tm.flush_older == 2 && c.open && !c.len && last_seen < a.tm.t) {
          c.close(GPK_TCPASM_CALL_FLUSH | r);
          flushed = closed = true;
        }
        if (lane == 0) {
          if (flushed) atomicAdd((unsigned long long*)&a.tm.counts[0], 1ull);
          if (closed) atomicAdd((unsigned long long*)&a.tm.counts[1], 1ull);
        }
      }
      if (lane == 0) a.tm.conn_last_seen[g] = c.open ? last_seen : INT64_MIN;
    }
    if (c.open) {
      c.end_stream(GPK_TCPASM_OPEN);
      for (uint32_t e = c.head + lane; e < c.head + c.len && e < (uint32_t)kSmallCap; e += 64) {
        c.gpkt[e] = s_pkt[e];  // the pages still listed: where pend_kernel reads them
        c.gmeta[e] = s_meta[e];
      }
    }
    if (lane == 0) {
      a.conn_seq[g] = c.open ? c.next : (int64_t)GPK_TCPASM_NO_CONN;
      a.w.g_creator[g] = c.open ? c.cr : kNone;
      a.w.g_npend[g] = c.open ? c.len : 0;
      a.w.g_head[g] = c.head;
    }
    for (uint32_t e = c.used + lane; e < cap; e += 64) c.wc[e].stream = kNone;  // slots no chunk took
    c.list_sync(0);  // the next key reuses the LDS list
  }
}

struct PageCount {  // by position in perm: the pages (= chunk slots) its packet can need
  const uint32_t* perm;
  const uint32_t* gcounts;
  const uint4* info;
  __host__ __device__ uint32_t operator()(uint32_t j) const {
    if (j >= gcounts[1]) return 0;
    const uint4 inf = info[perm[j]];
    return page_count(inf.y, inf.w);
  }
};
using PageIt = hipcub::TransformInputIterator<uint32_t, PageCount, hipcub::CountingInputIterator<uint32_t>>;

__global__ void __launch_bounds__(256) finish_kernel(const int32_t* group_of, const uint32_t* gcounts, uint64_t n,
                                                     Work w, gpk_tcp_streams o) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t G = gcounts[0];
  // Sum of caplens > data_bytes (packets that share bytes): the workspace bound
  // does not hold, nothing was planned. counts[7] says so, all else is empty.
  const bool bad = w.wbase[gcounts[1]] > w.wcap;
  bool is_open = false;
  if (i < n) {
    const int32_t g = group_of[i];
    if (g < 0) o.verdict[i] = g;
    if (bad && g >= 0) o.verdict[i] = GPK_TCPASM_NOCONN;
    const uint32_t c = bad ? kNone : w.creator[i];
    o.stream_of[i] = c == kNone ? -1 : (int32_t)w.snum[c];
    const uint32_t made = bad ? 0 : w.s_made[i], j = bad ? 0 : w.snum[i];
    if (made) {
      o.stream_group[j] = w.s_group[i];
      o.stream_first[j] = (uint32_t)i;
      o.stream_closed[j] = w.s_closed[i];
      o.stream_chunk0[j] = w.cbase[i];
      o.stream_data0[j] = w.dbase[i];
    }
    if (i < G) {
      const uint32_t gc = bad ? kNone : w.g_creator[i];
      o.conn_stream[i] = gc == kNone ? -1 : (int32_t)w.snum[gc];
      if (bad) o.conn_seq[i] = GPK_TCPASM_NO_CONN;
      is_open = gc != kNone;
      if (i + 1 == G) o.counts[3] = bad ? 0 : w.pbase[i] + w.g_npend[i];
    }
    if (i + 1 == n) {
      const uint32_t S = j + made, C = bad ? 0 : w.cbase[i] + w.s_nchunks[i];
      const uint64_t D = bad ? 0 : w.dbase[i] + w.s_nbytes[i];
      o.stream_chunk0[S] = C;
      o.stream_data0[S] = D;
      o.counts[0] = S;
      o.counts[1] = C;
      o.counts[2] = D;
      o.counts[5] = C > o.chunk_cap ? C - o.chunk_cap : 0;
      o.counts[6] = D > o.data_cap;
      o.counts[7] = bad;
    }
  }
  const uint64_t m = __ballot(is_open);
  if (m && (threadIdx.x & 63) == 0) atomicAdd((unsigned long long*)&o.counts[4], (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256) pend_kernel(const uint32_t* start, const uint32_t* gcounts, Work w,
                                                   gpk_tcp_streams o) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  const uint32_t G = gcounts[0];
  if (w.wbase[gcounts[1]] > w.wcap) return;
  for (uint32_t g = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); g < G; g += waves) {
    const uint32_t np = w.g_npend[g];
    if (!np) continue;
    const uint32_t from = w.wbase[start[g]] + w.g_head[g], to = w.pbase[g];
    for (uint32_t e = lane; e < np; e += 64)
      if ((uint64_t)to + e < o.chunk_cap) {
        o.pend_pkt[to + e] = w.pg_pkt[from + e];
        o.pend_page[to + e] = w.pg_meta[from + e] & 0xFFFFu;
      }
  }
}

struct EmitArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* gcounts;
  Work w;
  gpk_tcp_streams o;
};

__global__ void __launch_bounds__(256) emit_kernel(EmitArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  const uint32_t W = a.w.wbase[a.gcounts[1]];  // workspace slots in use
  if (W > a.w.wcap) return;
  for (uint32_t slot = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); slot < W; slot += waves) {
    gpk_tcp_chunk c = a.w.wc[slot];
    const uint32_t cr = c.stream;
    if (cr == kNone) continue;
    const uint64_t at = a.w.dbase[cr];
    const uint64_t idx = (uint64_t)a.w.cbase[cr] + (slot - a.w.s_wk0[cr]);
    const uint64_t local = c.dst;
    if (lane == 0 && idx < a.o.chunk_cap) {
      c.dst = at + local;
      c.stream = a.w.snum[cr];
      a.o.chunks[idx] = c;
    }
    if (!c.len || at + a.w.s_nbytes[cr] > a.o.data_cap) continue;  // a stream that does not fit is not written at all
    gpk::copy_bytes(a.o.data + at + local, a.data + a.offsets[c.src] + a.w.info[c.src].z + c.src_off, c.len, lane);
  }
}

}  // namespace

struct gpk_tcpasm {
  int device = 0;
  uint64_t cap = 0;
  Work w{};
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  gpk::Workspace ws;      // the arrays by packet: fixed at create
  gpk::Workspace slices;  // the arrays by workspace slot: replaced when a batch needs more slots
};

namespace {

void carve(gpk_tcpasm* d) {
  Work& w = d->w;
  gpk::Workspace& ws = d->ws;
  const uint64_t n = d->cap;
  ws.take(w.info, n), ws.take(w.creator, n), ws.take(w.s_made, n), ws.take(w.s_nchunks, n), ws.take(w.s_nbytes, n);
  ws.take(w.s_wk0, n), ws.take(w.s_closed, n), ws.take(w.s_group, n), ws.take(w.snum, n), ws.take(w.cbase, n);
  ws.take(w.dbase, n), ws.take(w.g_creator, n), ws.take(w.g_npend, n), ws.take(w.g_head, n), ws.take(w.pbase, n);
  ws.take(w.wbase, n + 1), ws.take(d->tmp, d->tmp_bytes);
}

void carve_slices(gpk_tcpasm* d, uint64_t wcap) {
  Work& w = d->w;
  d->slices.take(w.wc, wcap), d->slices.take(w.pg_seq, wcap), d->slices.take(w.pg_pkt, wcap);
  d->slices.take(w.pg_meta, wcap);
}

bool alloc_slices(gpk_tcpasm* d, uint64_t wcap) {  // replaces them; on failure the handle has none (wcap 0)
  d->slices.release();
  carve_slices(d, wcap);
  const bool ok = d->slices.alloc();
  carve_slices(d, wcap);
  d->w.wcap = ok ? wcap : 0;
  return ok;
}

}  // namespace

extern "C" int gpk_tcpasm_create(gpk_tcpasm** out, int device, uint64_t max_packets) {
  if (const int rc = gpk::check_create(out, device, max_packets)) return rc;
  gpk::DeviceScope dscope(device);  // the caller's device is restored on return
  if (dscope.err != hipSuccess) return GPK_EHIP;
  gpk_tcpasm* d = new (std::nothrow) gpk_tcpasm();
  if (!d) return GPK_ENOMEM;
  d->device = device;
  d->cap = max_packets;
  const uint64_t n = max_packets;
  size_t b0 = 0, b1 = 0, b2 = 0;
  bool ok = hipcub::DeviceScan::ExclusiveSum(
                nullptr, b0, PageIt(hipcub::CountingInputIterator<uint32_t>(0), PageCount{nullptr, nullptr, nullptr}),
                (uint32_t*)nullptr, (int)n + 1) == hipSuccess &&
            hipcub::DeviceScan::ExclusiveSum(nullptr, b1, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n) ==
                hipSuccess &&
            hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n) ==
                hipSuccess;
  d->tmp_bytes = gpk::max_temp({b0, b1, b2});
  carve(d);
  if (!ok || !d->ws.alloc() || !alloc_slices(d, 2 * n)) {
    d->ws.release();
    delete d;
    return GPK_ENOMEM;
  }
  carve(d);
  *out = d;
  return GPK_OK;
}

extern "C" int gpk_tcpasm_destroy(gpk_tcpasm* d) {
  if (!d) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  (void)hipDeviceSynchronize();
  d->slices.release();
  d->ws.release();
  delete d;
  return GPK_OK;
}

namespace {

// tm == nullptr: gpk_tcpasm_batch
int tcpasm_run(gpk_tcpasm* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g, const gpk_tcpasm_opts* op,
               const gpk_tcp_streams* o, const gpk_tcpasm_time* tm, void* stream) {
  if (!d || !b || !r || !g || !op || !o || !o->counts) return GPK_EINVAL;
  if (tm && (!tm->counts || tm->flush_older > 2 || (tm->flush_older && op->flush))) return GPK_EINVAL;
  const uint64_t n = b->n;
  if (n > d->cap || op->carried > n) return GPK_EINVAL;
  if (op->carried && (!op->carry_code || !op->carry_seq)) return GPK_EINVAL;
  if (n && (!b->data || !b->offsets || !r->layouts || !g->group_of || !g->perm || !g->start || !g->counts ||
            !o->verdict || !o->stream_of || !o->stream_group || !o->stream_first || !o->stream_closed ||
            !o->stream_chunk0 || !o->stream_data0 || !o->conn_seq || !o->conn_stream ||
            (o->chunk_cap && (!o->chunks || !o->pend_pkt || !o->pend_page)) || (!o->data && o->data_cap)))
    return GPK_EINVAL;
  if (tm && n && (!tm->seen || !tm->conn_last_seen)) return GPK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (hipMemsetAsync(o->counts, 0, 8 * sizeof(uint64_t), s) != hipSuccess) return GPK_EHIP;
  if (tm && hipMemsetAsync(tm->counts, 0, 2 * sizeof(uint64_t), s) != hipSuccess) return GPK_EHIP;
  if (o->stream_chunk0 && hipMemsetAsync(o->stream_chunk0, 0, sizeof(uint32_t), s) != hipSuccess) return GPK_EHIP;
  if (o->stream_data0 && hipMemsetAsync(o->stream_data0, 0, sizeof(uint64_t), s) != hipSuccess) return GPK_EHIP;
  if (n == 0) return GPK_OK;
  const uint64_t want_w = n + b->data_bytes / kPage;
  if (want_w >= (1ull << 32)) return GPK_EINVAL;
  if (want_w > d->w.wcap) {  // the workspace serves one call at a time: nothing of it is in flight
    if (hipDeviceSynchronize() != hipSuccess) return GPK_EHIP;
    if (!alloc_slices(d, want_w)) return GPK_ENOMEM;
  }
  const Work& w = d->w;
  const dim3 blk(256), grd((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(prep_kernel, grd, blk, 0, s, b->data, b->offsets, r->layouts, g->group_of, n, op->carried,
                     op->carry_code, w);
  size_t tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(
          d->tmp, tb, PageIt(hipcub::CountingInputIterator<uint32_t>(0), PageCount{g->perm, g->counts, w.info}),
          w.wbase, (int)n + 1, s) != hipSuccess)
    return GPK_EHIP;
  // one wave per key, striding: at most n keys
  const unsigned pblocks = (unsigned)std::min<uint64_t>(n, 1u << 18);
  const PlanArgs pa{g->perm,       g->start,   g->counts,   op->carry_seq, op->max_pages,
                    op->flush,     o->verdict, o->conn_seq, w,             tm ? *tm : gpk_tcpasm_time{}};
  if (tm) {
    hipLaunchKernelGGL((plan_kernel<true, true>), dim3(pblocks), dim3(64), 0, s, pa);
    hipLaunchKernelGGL((plan_kernel<false, true>), dim3(std::min(pblocks, 4096u)), dim3(64), 0, s, pa);
  } else {
    hipLaunchKernelGGL((plan_kernel<true, false>), dim3(pblocks), dim3(64), 0, s, pa);
    hipLaunchKernelGGL((plan_kernel<false, false>), dim3(std::min(pblocks, 4096u)), dim3(64), 0, s, pa);
  }
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, (const uint32_t*)w.s_made, w.snum, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, (const uint32_t*)w.s_nchunks, w.cbase, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, (const uint64_t*)w.s_nbytes, w.dbase, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, (const uint32_t*)w.g_npend, w.pbase, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  hipLaunchKernelGGL(finish_kernel, grd, blk, 0, s, g->group_of, g->counts, n, w, *o);
  const uint64_t gwant = (n + 3) / 4;  // 4 waves per block
  hipLaunchKernelGGL(pend_kernel, dim3((unsigned)std::min<uint64_t>(gwant, 16384)), blk, 0, s, g->start, g->counts, w,
                     *o);
  const uint64_t want = (w.wcap + 3) / 4;
  const EmitArgs ea{b->data, b->offsets, g->counts, w, *o};
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)std::min<uint64_t>(want, 65536)), blk, 0, s, ea);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

}  // namespace

extern "C" int gpk_tcpasm_batch(gpk_tcpasm* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g,
                                const gpk_tcpasm_opts* op, const gpk_tcp_streams* o, void* stream) {
  return tcpasm_run(d, b, r, g, op, o, nullptr, stream);
}

extern "C" int gpk_tcpasm_batch_timed(gpk_tcpasm* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g,
                                      const gpk_tcpasm_opts* op, const gpk_tcp_streams* o, const gpk_tcpasm_time* tm,
                                      void* stream) {
  if (!tm) return GPK_EINVAL;
  return tcpasm_run(d, b, r, g, op, o, tm, stream);
}
