// gpk_defrag.hip — IPv4 reassembly of a decoded, defrag-grouped batch
// (include/gpk_defrag.h): ip4defrag's fragmentList.insert / build and the tail
// of DefragIPv4WithTimestamp for every key of a batch, then the byte movement.
//
//   1. prep_kernel   one lane per packet: the IPv4 fields the state machine
//                    reads (FragOffset, Length, MF, IHL, the payload's length
//                    as the decode sliced it), once, in 16 bytes
//   2. plan_kernel   one wave per key (group), its packets in batch order. The
//                    fragment list lives in LDS; the wave looks a fragment up
//                    64 list entries at a time by ballot (the first entry that
//                    is equal or larger decides, as the reference's scan does)
//                    and shifts the tail in parallel for an insert. build walks
//                    the list in order: 64 entries' fields are gathered at once,
//                    then read lane by lane. A built datagram leaves its list
//                    in the key's own slice of an n-entry workspace as segment
//                    descriptors: a packet enters at most one list instance, so
//                    the slice always has room. Two instantiations: keys of up
//                    to 64 packets (a 64-entry list) and the rest (8192 entries,
//                    the reference's maximum).
//   3. hipcub scans  datagram numbers, byte offsets, pending positions
//   4. finish_kernel per-datagram arrays, verdicts, pending list, counts
//   5. copy_kernel   one wave per segment: destination-aligned 16-byte stores,
//                    the source realigned in registers, a byte head and tail.
//                    The wave of a datagram's first segment also writes its
//                    header. A datagram is split at its fragments, so no work
//                    item is longer than one fragment's payload (64 KB at most,
//                    64 wave steps; 2 at MTU 1500).
//   time (gpk_defrag_batch_timed) adds four small kernels around the scans and
//   leaves the five above as they are: `pending` lists exactly the fragments
//   that stamped LastSeen, in arrival order, so a key's LastSeen is seen[] of
//   its last pending packet. mark_kernel finds that packet per key (an atomic
//   maximum over the key's pending packets, and their count), key_kernel turns
//   it into the key's LastSeen and the discard decision and counts, drop_kernel
//   takes a discarded key's packets out of `pending` before the scan, and
//   seen_kernel writes pending_seen behind it.
// Every list state variable is computed identically by all 64 lanes from
// shuffled values, so the control flow around ballots, shuffles and barriers
// is wave-uniform; blocks of the plan kernel are one wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>

#include "../../include/gpk_defrag.h"
#include "gpk_copy.h"
#include "gpk_scan.h"
#include "gpk_workspace.h"

namespace {

constexpr int kSlotIp4 = 2;  // gpk_layout slot of IPv4
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;
constexpr uint32_t kFirstSeg = 1u << 31;  // in seg_skip: the datagram's first segment
constexpr int kSmallCap = 64;
constexpr int32_t kBuilt = 0;

// info[i]: x = FragOffset | Length << 16, y = len(Payload) | MF << 16 | IHL << 17,
//          z = IPv4 start in the packet, w = end of the IPv4 header in the packet
struct Work {
  uint4* info;
  uint32_t* inst;       // [n] 0: never counted; else 1 + flushes of its key before it was counted
  uint32_t* final_inst; // [n] per group: 1 + flushes of the key in this batch
  uint32_t* dsize;      // [n] bytes of the datagram this packet completed, or 0
  uint32_t* dhigh;      // [n] its Highest
  uint32_t* dnum;       // [n] scan: datagram number
  uint64_t* ddst;       // [n] scan: datagram byte offset
  uint32_t* ppos;       // [n] scan: position in pending
  uint32_t* seg_pkt;    // [n] per workspace slot: source packet
  uint32_t* seg_skip;   // [n]   bytes of its payload skipped (startAt) | kFirstSeg
  uint32_t* seg_dst;    // [n]   offset inside the datagram's payload
  uint32_t* seg_owner;  // [n]   the packet that completed the datagram, or kNoOwner
};

__global__ void __launch_bounds__(256) prep_kernel(const uint8_t* data, const uint64_t* offsets,
                                                   const gpk_layout* layouts, const int32_t* group_of, uint64_t n,
                                                   Work w) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w.inst[i] = 0;
  w.dsize[i] = 0;
  w.dhigh[i] = 0;
  w.seg_owner[i] = kNoOwner;
  uint4 inf = make_uint4(0, 0, 0, 0);
  if (group_of[i] >= 0) {  // keyed: the IPv4 slot holds a successful decode of >= 20 bytes
    const uint32_t s = layouts[i].start[kSlotIp4], len = layouts[i].end[kSlotIp4] - s;
    const uint8_t* ip = data + offsets[i] + s;
    uint32_t length = (uint32_t)ip[2] << 8 | ip[3];
    if (length == 0) length = len & 0xFFFF;  // ip4.go:189-193
    const uint32_t ihl = ip[0] & 15u;
    const uint32_t ff = (uint32_t)ip[6] << 8 | ip[7];
    const uint32_t avail = len < length ? len : length;  // ip4.go:203-214
    const uint32_t paylen = avail > ihl * 4 ? avail - ihl * 4 : 0;
    inf = make_uint4((ff & 0x1FFF) | length << 16, paylen | ((ff >> 13) & 1u) << 16 | ihl << 17, s, s + ihl * 4);
  }
  w.info[i] = inf;
}

struct PlanArgs {
  const uint32_t* perm;
  const uint32_t* start;
  const uint32_t* gcounts;
  int32_t* verdict;
  Work w;
};

template <int CAP>
__global__ void __launch_bounds__(64) plan_kernel(PlanArgs a) {
  __shared__ uint32_t l_pkt[CAP];
  __shared__ uint16_t l_fo[CAP];
  const uint32_t lane = threadIdx.x;
  const uint32_t G = a.gcounts[0];
  for (uint32_t g = blockIdx.x; g < G; g += gridDim.x) {
    const uint32_t s = a.start[g], k = a.start[g + 1] - s;
    if ((k <= (uint32_t)kSmallCap) != (CAP == kSmallCap)) continue;
    uint32_t len = 0, highest = 0, current = 0, fin = 0, used = 0, flushes = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += 64) {
      const uint32_t cnt = k - c0 < 64 ? k - c0 : 64;
      uint32_t pkt = 0;
      uint4 inf = make_uint4(0, 0, 0, 0);
      if (lane < cnt) {
        pkt = a.perm[s + c0 + lane];
        inf = a.w.info[pkt];
      }
      int32_t my_v = GPK_DEFRAG_HELD;
      uint32_t my_inst = 0, my_size = 0, my_high = 0;
      for (uint32_t t = 0; t < cnt; t++) {
        const uint32_t x = (uint32_t)__shfl((int)inf.x, (int)t), y = (uint32_t)__shfl((int)inf.y, (int)t);
        const uint32_t tp = (uint32_t)__shfl((int)pkt, (int)t), thdr = (uint32_t)__shfl((int)inf.w, (int)t);
        const uint32_t fo = x & 0xFFFF, length = x >> 16, off8 = fo * 8;
        const uint32_t frag_len = (length - 20) & 0xFFFF;
        int32_t v = GPK_DEFRAG_HELD;
        bool counted = true;
        // ---- insert (defrag.go:217-247)
        if (off8 >= highest) {
          if (lane == 0 && len < (uint32_t)CAP) {
            l_pkt[len] = tp;
            l_fo[len] = (uint16_t)fo;
          }
          len++;
          __syncthreads();
        } else {
          int pos = -1;
          for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t e = base + lane;
            const bool val = e < len;
            const uint32_t efo = val ? l_fo[e] : 0;
            const uint64_t md = __ballot(val && efo == fo), mb = __ballot(val && efo > fo);
            if (md | mb) {
              const int f = __builtin_ctzll(md | mb);
              if ((md >> f) & 1)
                counted = false;  // "ignoring frag as we already have it": (nil, nil)
              else
                pos = (int)(base + f);
              break;
            }
          }
          if (pos >= 0) {  // InsertBefore: move [pos, len) up by one, from the tail
            for (uint32_t hi = len; hi > (uint32_t)pos;) {
              const uint32_t lo = hi - (uint32_t)pos > 64 ? hi - 64 : (uint32_t)pos;
              const uint32_t e = lo + lane;
              const bool val = e < hi && e + 1 < (uint32_t)CAP;
              const uint32_t vp = val ? l_pkt[e] : 0;
              const uint16_t vf = val ? l_fo[e] : (uint16_t)0;
              __syncthreads();
              if (val) {
                l_pkt[e + 1] = vp;
                l_fo[e + 1] = vf;
              }
              __syncthreads();
              hi = lo;
            }
            if (lane == 0) {
              l_pkt[pos] = tp;
              l_fo[pos] = (uint16_t)fo;
            }
            len++;
            __syncthreads();
          }
          // no larger offset: not listed, the counters move all the same
        }
        uint32_t total = 0;
        if (counted) {  // :249-270
          const uint32_t hi16 = (off8 + frag_len) & 0xFFFF;
          if (highest < hi16) highest = hi16;
          current = (current + frag_len) & 0xFFFF;
          if (!((y >> 16) & 1u)) fin = 1;
          if (fin && highest == current) {
            // ---- build (:276-304)
            uint32_t cur = 0;
            v = kBuilt;
            for (uint32_t base = 0; base < len && v == kBuilt; base += 64) {
              const uint32_t e = base + lane;
              const uint32_t bc = len - base < 64 ? len - base : 64;
              uint4 ei = make_uint4(0, 0, 0, 0);
              if (lane < bc) ei = a.w.info[l_pkt[e]];
              uint32_t my_skip = 0, my_dst = 0;
              for (uint32_t j = 0; j < bc; j++) {
                const uint32_t ex = (uint32_t)__shfl((int)ei.x, (int)j);
                const uint32_t epl = (uint32_t)__shfl((int)ei.y, (int)j) & 0xFFFF;
                const uint32_t eo = (ex & 0xFFFF) * 8, el = ex >> 16;
                uint32_t skip = 0;
                if (eo == cur) {
                  cur = (cur + el - 20) & 0xFFFF;
                } else if (eo < cur) {
                  skip = cur - eo;
                  if (skip > ((el - 20) & 0xFFFF)) {
                    v = GPK_DEFRAG_EINVALID;
                    break;
                  }
                  if (skip > epl) {  // frag.Payload[startAt:] panics
                    v = GPK_DEFRAG_EPANIC;
                    break;
                  }
                  cur = (cur + eo) & 0xFFFF;
                } else {
                  v = GPK_DEFRAG_EHOLE;
                  break;
                }
                if (lane == j) {
                  my_skip = skip | (base + j == 0 ? kFirstSeg : 0u);
                  my_dst = total;
                }
                total += epl - skip;
              }
              // optimistic: owners are set only once the whole list has built
              if (lane < bc && used + e < k) {
                a.w.seg_skip[s + used + e] = my_skip;
                a.w.seg_dst[s + used + e] = my_dst;
              }
            }
          }
        }
        const uint32_t inst_t = counted ? flushes + 1 : 0;
        const uint32_t high_t = highest;
        if (v == kBuilt) {  // :126-131: the list becomes the datagram's segments, the key starts again
          for (uint32_t e = lane; e < len; e += 64)
            if (used + e < k) {
              a.w.seg_pkt[s + used + e] = l_pkt[e];
              a.w.seg_owner[s + used + e] = tp;
            }
          used += len;
        } else if (len + 1 > GPK_DEFRAG_MAX_LIST) {  // :118-123
          v = GPK_DEFRAG_EMAXLEN;
        }
        if (v == kBuilt || v == GPK_DEFRAG_EMAXLEN) {  // flush
          __syncthreads();
          len = highest = current = fin = 0;
          flushes++;
        }
        if (lane == t) {
          my_v = v;
          my_inst = inst_t;
          if (v == kBuilt) {
            my_size = thdr + total;
            my_high = high_t;
          }
        }
      }
      if (lane < cnt) {
        a.verdict[pkt] = my_v;
        a.w.inst[pkt] = my_inst;
        if (my_size) {
          a.w.dsize[pkt] = my_size;
          a.w.dhigh[pkt] = my_high;
        }
      }
    }
    if (lane == 0) a.w.final_inst[g] = flushes + 1;
    __syncthreads();
  }
}

struct IsPending {  // counted for the instance of its key that is still open at the end of the batch
  const uint32_t* inst;
  const uint32_t* final_inst;
  const int32_t* group_of;
  __host__ __device__ uint32_t operator()(uint32_t i) const {
    const uint32_t v = inst[i];
    return v != 0 && v == final_inst[group_of[i]];
  }
};
using DnumIt = hipcub::TransformInputIterator<uint32_t, NonZero, const uint32_t*>;
using DdstIt = hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*>;
using PendIt = hipcub::TransformInputIterator<uint32_t, IsPending, hipcub::CountingInputIterator<uint32_t>>;

__global__ void __launch_bounds__(256) finish_kernel(const int32_t* group_of, uint64_t n, Work w, IsPending pend,
                                                     gpk_datagrams o) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = group_of[i];
  if (g < 0) o.verdict[i] = g;
  const uint32_t sz = w.dsize[i], j = w.dnum[i];
  const uint64_t at = w.ddst[i];
  if (sz) {
    o.verdict[i] = (int32_t)j;
    o.last[j] = (uint32_t)i;
    o.length[j] = w.dhigh[i];
    o.offsets[j] = at;
    o.caplens[j] = sz;
    o.payload_off[j] = w.info[i].w;
  }
  const uint32_t p = g >= 0 ? pend((uint32_t)i) : 0u;
  if (p) o.pending[w.ppos[i]] = (uint32_t)i;
  if (i + 1 == n) {
    o.counts[0] = j + (sz != 0);
    o.counts[1] = w.ppos[i] + p;
    o.counts[2] = at + sz;
    o.counts[3] = at + sz > o.data_cap;
  }
}

// ---- time: LastSeen and DiscardOlderThan (defrag.go:138-149, :249)
struct TimeWork {
  uint32_t* key_last;  // [n] per group: 1 + its last pending packet, 0 if it has none
  uint32_t* key_cnt;   // [n] per group: its pending packets
  int64_t* key_seen;   // [n] per group: LastSeen
  uint32_t* dead;      // [n] per group: discarded
};

__global__ void __launch_bounds__(256) mark_kernel(const int32_t* group_of, uint64_t n, IsPending pend, TimeWork tw) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = group_of[i];
  if (g < 0 || !pend((uint32_t)i)) return;
  atomicMax(&tw.key_last[g], (uint32_t)i + 1);
  atomicAdd(&tw.key_cnt[g], 1u);
}

__global__ void __launch_bounds__(256) key_kernel(const uint32_t* gcounts, uint64_t n, TimeWork tw,
                                                  gpk_defrag_time tm) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = g < n && g < gcounts[0];
  uint32_t dead = 0, dropped = 0;
  if (live) {
    const uint32_t last = tw.key_last[g];
    int64_t ks = INT64_MIN;  // a key flushed by the end of the batch: nothing pending, nothing to discard
    if (last) {
      ks = tm.seen[last - 1];
      dead = tm.discard && ks < tm.t;
      if (dead) dropped = tw.key_cnt[g];
    }
    tw.key_seen[g] = ks;
    tw.dead[g] = dead;
  }
  const uint32_t keys = (uint32_t)__popcll(__ballot(dead != 0));
  for (int m = 32; m; m >>= 1) dropped += (uint32_t)__shfl_xor((int)dropped, m);
  if ((threadIdx.x & 63) == 0 && keys) {
    atomicAdd((unsigned long long*)&tm.counts[0], (unsigned long long)keys);
    atomicAdd((unsigned long long*)&tm.counts[1], (unsigned long long)dropped);
  }
}

__global__ void __launch_bounds__(256) drop_kernel(const int32_t* group_of, uint64_t n, TimeWork tw, uint32_t* inst) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = group_of[i];
  if (g >= 0 && tw.dead[g]) inst[i] = 0;  // no longer counted for a live key
}

__global__ void __launch_bounds__(256) seen_kernel(const int32_t* group_of, uint64_t n, IsPending pend,
                                                   const uint32_t* ppos, TimeWork tw, int64_t* pending_seen) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = group_of[i];
  if (g >= 0 && pend((uint32_t)i)) pending_seen[ppos[i]] = tw.key_seen[g];
}

using gpk::copy_bytes;  // gpk_copy.h

struct CopyArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  const uint32_t* gcounts;
  Work w;
  uint8_t* out;
  uint64_t cap;
};

__global__ void __launch_bounds__(256) copy_kernel(CopyArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  const uint32_t K = a.gcounts[1];  // keyed packets: the workspace slots in use
  for (uint32_t slot = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); slot < K; slot += waves) {
    const uint32_t owner = a.w.seg_owner[slot];
    if (owner == kNoOwner) continue;
    const uint64_t at = a.w.ddst[owner];
    const uint32_t size = a.w.dsize[owner];
    if (at + size > a.cap) continue;  // a datagram that does not fit is not written at all
    const uint4 oi = a.w.info[owner];
    const uint32_t hdr = oi.w;
    const uint32_t sk = a.w.seg_skip[slot], skip = sk & 0xFFFF;
    const uint32_t pkt = a.w.seg_pkt[slot];
    const uint4 pi = a.w.info[pkt];
    uint8_t* dgram = a.out + at;
    copy_bytes(dgram + hdr + a.w.seg_dst[slot], a.data + a.offsets[pkt] + pi.w + skip, (pi.y & 0xFFFF) - skip, lane);
    if (!(sk & kFirstSeg)) continue;
    // the header: `in` from the packet start through its IPv4 header, with
    // Flags/FragOffset 0, the datagram's Total Length and a fresh checksum
    const uint8_t* hs = a.data + a.offsets[owner];
    const uint32_t s = oi.z, ihl = (oi.y >> 17) & 15u;
    uint32_t tot = ihl * 4 + (size - hdr);
    if (tot > 0xFFFF) tot = 0;
    uint32_t sum = 0;
    if (lane < ihl * 2) {
      sum = (uint32_t)hs[s + 2 * lane] << 8 | hs[s + 2 * lane + 1];
      if (lane == 1) sum = tot;
      if (lane == 3 || lane == 5) sum = 0;
    }
    for (int m = 32; m; m >>= 1) sum += (uint32_t)__shfl_xor((int)sum, m);
    sum = (sum & 0xFFFF) + (sum >> 16);
    sum = (sum & 0xFFFF) + (sum >> 16);
    const uint32_t ck = ~sum & 0xFFFF;
    for (uint32_t b = lane; b < hdr; b += 64) {
      uint32_t v = hs[b];
      const uint32_t rel = b - s;  // wraps for the bytes before the IPv4 header
      if (rel == 2) v = tot >> 8;
      if (rel == 3) v = tot & 0xFF;
      if (rel == 6 || rel == 7) v = 0;
      if (rel == 10) v = ck >> 8;
      if (rel == 11) v = ck & 0xFF;
      dgram[b] = (uint8_t)v;
    }
  }
}

}  // namespace

struct gpk_defragger {
  int device = 0;
  uint64_t cap = 0;
  Work w{};
  TimeWork tw{};
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  gpk::Workspace ws;
};

namespace {

void carve(gpk_defragger* d) {  // every device array of the handle
  const uint64_t n = d->cap;
  d->ws.take(d->w.info, n), d->ws.take(d->w.inst, n), d->ws.take(d->w.final_inst, n), d->ws.take(d->w.dsize, n);
  d->ws.take(d->w.dhigh, n), d->ws.take(d->w.dnum, n), d->ws.take(d->w.ddst, n), d->ws.take(d->w.ppos, n);
  d->ws.take(d->w.seg_pkt, n), d->ws.take(d->w.seg_skip, n), d->ws.take(d->w.seg_dst, n);
  d->ws.take(d->w.seg_owner, n), d->ws.take(d->tw.key_last, n), d->ws.take(d->tw.key_cnt, n);
  d->ws.take(d->tw.key_seen, n), d->ws.take(d->tw.dead, n), d->ws.take(d->tmp, d->tmp_bytes);
}

}  // namespace

extern "C" int gpk_defragger_create(gpk_defragger** out, int device, uint64_t max_packets) {
  if (const int rc = gpk::check_create(out, device, max_packets)) return rc;
  gpk::DeviceScope dscope(device);  // the caller's device is restored on return
  if (dscope.err != hipSuccess) return GPK_EHIP;
  gpk_defragger* d = new (std::nothrow) gpk_defragger();
  if (!d) return GPK_ENOMEM;
  d->device = device;
  d->cap = max_packets;
  const uint64_t n = max_packets;
  size_t b0 = 0, b1 = 0, b2 = 0;
  bool ok = hipcub::DeviceScan::ExclusiveSum(nullptr, b0, DnumIt(nullptr, NonZero()), (uint32_t*)nullptr, (int)n) ==
                hipSuccess &&
            hipcub::DeviceScan::ExclusiveSum(nullptr, b1, DdstIt(nullptr, Widen()), (uint64_t*)nullptr, (int)n) ==
                hipSuccess &&
            hipcub::DeviceScan::ExclusiveSum(
                nullptr, b2, PendIt(hipcub::CountingInputIterator<uint32_t>(0), IsPending{nullptr, nullptr, nullptr}),
                (uint32_t*)nullptr, (int)n) == hipSuccess;
  d->tmp_bytes = gpk::max_temp({b0, b1, b2});
  carve(d);
  if (!ok || !d->ws.alloc()) {
    delete d;
    return GPK_ENOMEM;
  }
  carve(d);
  *out = d;
  return GPK_OK;
}

extern "C" int gpk_defragger_destroy(gpk_defragger* d) {
  if (!d) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  (void)hipDeviceSynchronize();
  d->ws.release();
  delete d;
  return GPK_OK;
}

namespace {

// tm == nullptr: gpk_defrag_batch
int defrag_run(gpk_defragger* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g, const gpk_datagrams* o,
               const gpk_defrag_time* tm, void* stream) {
  if (!d || !b || !r || !g || !o || !o->counts) return GPK_EINVAL;
  const uint64_t n = b->n;
  if (n > d->cap) return GPK_EINVAL;
  if (n && (!b->data || !b->offsets || !r->layouts || !g->group_of || !g->perm || !g->start || !g->counts ||
            !o->verdict || !o->last || !o->length || !o->offsets || !o->caplens || !o->payload_off || !o->pending ||
            (!o->data && o->data_cap)))
    return GPK_EINVAL;
  if (tm && (!tm->counts || (n && (!tm->seen || !tm->pending_seen)))) return GPK_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  gpk::DeviceScope dscope(d->device);
  if (dscope.err != hipSuccess) return GPK_EHIP;
  if (hipMemsetAsync(o->counts, 0, 4 * sizeof(uint64_t), s) != hipSuccess) return GPK_EHIP;
  if (tm && hipMemsetAsync(tm->counts, 0, 2 * sizeof(uint64_t), s) != hipSuccess) return GPK_EHIP;
  if (n == 0) return GPK_OK;
  const Work& w = d->w;
  const dim3 blk(256), grd((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(prep_kernel, grd, blk, 0, s, b->data, b->offsets, r->layouts, g->group_of, n, w);
  // one wave per key, striding: at most n keys
  const unsigned pblocks = (unsigned)std::min<uint64_t>(n, 1u << 18);
  const PlanArgs pa{g->perm, g->start, g->counts, o->verdict, w};
  hipLaunchKernelGGL(plan_kernel<kSmallCap>, dim3(pblocks), dim3(64), 0, s, pa);
  hipLaunchKernelGGL(plan_kernel<GPK_DEFRAG_MAX_LIST>, dim3(std::min(pblocks, 4096u)), dim3(64), 0, s, pa);
  const IsPending pend{w.inst, w.final_inst, g->group_of};
  if (tm) {
    const TimeWork& tw = d->tw;
    if (hipMemsetAsync(tw.key_last, 0, n * 4, s) != hipSuccess || hipMemsetAsync(tw.key_cnt, 0, n * 4, s) != hipSuccess)
      return GPK_EHIP;
    hipLaunchKernelGGL(mark_kernel, grd, blk, 0, s, g->group_of, n, pend, tw);
    hipLaunchKernelGGL(key_kernel, grd, blk, 0, s, g->counts, n, tw, *tm);
    if (tm->discard) hipLaunchKernelGGL(drop_kernel, grd, blk, 0, s, g->group_of, n, tw, w.inst);
  }
  size_t tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, DnumIt(w.dsize, NonZero()), w.dnum, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, DdstIt(w.dsize, Widen()), w.ddst, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, PendIt(hipcub::CountingInputIterator<uint32_t>(0), pend), w.ppos,
                                       (int)n, s) != hipSuccess)
    return GPK_EHIP;
  hipLaunchKernelGGL(finish_kernel, grd, blk, 0, s, g->group_of, n, w, pend, *o);
  if (tm) hipLaunchKernelGGL(seen_kernel, grd, blk, 0, s, g->group_of, n, pend, w.ppos, d->tw, tm->pending_seen);
  const uint64_t want = (n + 3) / 4;  // 4 waves per block, one segment per wave per pass
  const CopyArgs ca{b->data, b->offsets, g->counts, w, o->data, o->data_cap};
  hipLaunchKernelGGL(copy_kernel, dim3((unsigned)std::min<uint64_t>(want, 65536)), blk, 0, s, ca);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

}  // namespace

extern "C" int gpk_defrag_batch(gpk_defragger* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g,
                                const gpk_datagrams* o, void* stream) {
  return defrag_run(d, b, r, g, o, nullptr, stream);
}

extern "C" int gpk_defrag_batch_timed(gpk_defragger* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g,
                                      const gpk_datagrams* o, const gpk_defrag_time* tm, void* stream) {
  if (!tm) return GPK_EINVAL;
  return defrag_run(d, b, r, g, o, tm, stream);
}
