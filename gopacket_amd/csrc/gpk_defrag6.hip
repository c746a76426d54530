// gpk_defrag6.hip — IPv6 reassembly of a decoded, DEFRAG6-grouped batch
// (include/gpk_defrag6.h): ip6defrag's DefragIPv6 for every key of a batch,
// then the byte movement.
//
//   1. prep6_kernel  one lane per keyed packet: the walk to the Fragment header
//                    (gpk_frag6.h, the one the grouping keyed by), then the
//                    fields the state machine reads, in 16 bytes
//   2. plan6_kernel  one wave per key (group), its packets in batch order. The
//                    list lives in LDS, 8 bytes an entry; a fragment is looked up
//                    64 entries at a time by ballot (an equal entry, else the
//                    first larger one, decides) and an insert shifts the tail in
//                    parallel. The reference re-walks the chain from the head on
//                    every call; here the position of the chain's first stop (an
//                    entry with `more` unset, or whose successor is missing or
//                    does not line up) is kept: an insert behind it changes
//                    nothing, any other insert rescans from its predecessor by
//                    ballot. In-order traffic costs one step per fragment and a
//                    call after completion O(1). Two instantiations: keys of up to
//                    64 packets and the rest (8192 entries: 64 KB of LDS).
//                    Nothing is ever removed, so the list at the time of packet t
//                    is the key's FINAL list restricted to entries that arrived
//                    by t: the final list is left in the key's own slice of an
//                    n-entry workspace as packet indices (ascending arrival inside
//                    a key), and a datagram is (key, last packet).
//   3. hipcub scans  datagram numbers, byte offsets, pending positions
//   4. finish6       per-datagram arrays, verdicts, pending list, counts, and per
//                    datagram one 32-byte descriptor for the mover
//   5. move6_kernel  one block of four waves per datagram. A wave reads the
//                    descriptor, then walks the key's final list filtered by arrival
//                    (64 entries a step, their fields and source addresses gathered
//                    by the lanes at once) up to the first entry with `more` unset,
//                    and copies every fourth fragment (gpk_copy.h: destination-
//                    aligned 16-byte stores, the source realigned in registers). No
//                    work item is longer than one fragment's payload, re-emission
//                    needs no materialised segment lists, and a datagram's first
//                    byte is four dependent loads away. The last wave writes the
//                    header.
//   time (gpk_defrag6_batch_timed) adds three small kernels around the scans
//   and leaves the five above as they are: every call stamps its key, so a
//   key's time is seen[] of the key's last packet. key6_kernel reads it per key
//   and decides the discard, drop6_kernel takes a discarded key's fragments out
//   of `listed` before the pending scan, seen6_kernel writes pending_seen.
// Every list state variable is computed identically by all 64 lanes from
// shuffled values, so the control flow around ballots, shuffles and barriers
// is wave-uniform; blocks of the plan kernel are one wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>

#include "../../include/gpk_defrag6.h"
#include "gpk_copy.h"
#include "gpk_frag6.h"
#include "gpk_scan.h"
#include "gpk_workspace.h"

namespace {

constexpr int kSlotIp6 = 3;  // gpk_layout slot of IPv6
constexpr int kSmallCap = 64;
constexpr uint32_t kMore = 1u << 31;  // in a list entry's position word
constexpr uint32_t kPosMask = kMore - 1;

// info[i]: x = FragmentOffset | MoreFragments << 16 | NextHeader << 24,
//          y = fg.LayerPayload()'s start in the packet, z = its length,
//          w = the IPv6 header's start in the packet
struct Work {
  uint4* info;
  uint32_t* listed;   // [n] 1: its fragment was listed (not an ignored duplicate)
  uint32_t* dsize;    // [n] bytes of the datagram this packet's call returned, or 0
  uint32_t* dpay;     // [n]   of which payload
  uint32_t* dhead;    // [n]   the packet that gives the header
  uint32_t* dnum;     // [n] scan: datagram number
  uint64_t* ddst;     // [n] scan: datagram byte offset
  uint32_t* ppos;     // [n] scan: position in pending
  uint32_t* fin;      // [n] per key, in its slice of perm: the final list (packet indices)
  uint32_t* fin_len;  // [n] per key: its length
  uint4* desc;        // [2n] per datagram, all the mover needs in one read:
                      //      {offset lo, hi, bytes, payload_off}, {key's slice, its final list's length, last, head}
};

__global__ void __launch_bounds__(256) prep6_kernel(const uint8_t* data, const uint64_t* offsets,
                                                    const gpk_layout* layouts, const int32_t* group_of, uint64_t n,
                                                    Work w) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w.listed[i] = 0;
  w.dsize[i] = 0;
  uint4 inf = make_uint4(0, 0, 0, 0);
  if (group_of[i] >= 0) {  // keyed: the same walk found a Fragment header
    const uint32_t s = layouts[i].start[kSlotIp6];
    const uint8_t* ip = data + offsets[i] + s;
    gpk::Frag6 f;
    if (gpk::find_frag6(ip, layouts[i].end[kSlotIp6] - s, &f)) {
      const uint8_t* fh = ip + f.hdr;  // decodeIPv6Fragment, ip6.go:648-661
      const uint32_t fo = ((uint32_t)fh[2] << 8 | fh[3]) >> 3;
      inf = make_uint4(fo | (uint32_t)(fh[3] & 1u) << 16 | (uint32_t)fh[0] << 24, s + f.hdr + 8, f.end - (f.hdr + 8), s);
    }
  }
  w.info[i] = inf;
}

struct PlanArgs {
  const uint32_t* perm;
  const uint32_t* start;
  const uint32_t* gcounts;
  uint32_t carry;
  int32_t* verdict;
  Work w;
};

template <int CAP>
__global__ void __launch_bounds__(64) plan6_kernel(PlanArgs a) {
  __shared__ uint32_t l_pos[CAP];  // the fragment's position among the key's packets | kMore
  __shared__ uint32_t l_ol[CAP];   // offset | uint16(len(payload)/8) << 16
  const uint32_t lane = threadIdx.x;
  const uint32_t G = a.gcounts[0];
  for (uint32_t g = blockIdx.x; g < G; g += gridDim.x) {
    const uint32_t s = a.start[g], k = a.start[g + 1] - s;
    if ((k <= (uint32_t)kSmallCap) != (CAP == kSmallCap)) continue;
    uint32_t len = 0, stop = 0;   // stop: the first entry at which the walk from the head ends
    bool complete = false;        // the head's offset is 0 and the entry at `stop` has `more` unset
    bool fresh = false;           // c_* describe the datagram of the current list
    uint32_t c_pay = 0, c_head = 0, c_hdr = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += 64) {
      const uint32_t cnt = k - c0 < 64 ? k - c0 : 64;
      uint32_t pkt = 0;
      uint4 inf = make_uint4(0, 0, 0, 0);
      if (lane < cnt) {
        pkt = a.perm[s + c0 + lane];
        inf = a.w.info[pkt];
      }
      int32_t my_v = GPK_DEFRAG6_HELD;
      uint32_t my_listed = 0, my_size = 0, my_pay = 0, my_head = 0;
      for (uint32_t t = 0; t < cnt; t++) {
        const uint32_t x = (uint32_t)__shfl((int)inf.x, (int)t), plen = (uint32_t)__shfl((int)inf.z, (int)t);
        const uint32_t tp = (uint32_t)__shfl((int)pkt, (int)t);
        const uint32_t fo = x & 0x1FFF, T = c0 + t;
        const uint32_t e_pos = T | (((x >> 16) & 1u) ? kMore : 0u), e_ol = fo | ((plen >> 3) & 0xFFFFu) << 16;
        // ---- the list scan (defrag.go:107-129); the first call just stores (:98-103)
        int pos = -1;
        if (len == 0) {
          pos = 0;
        } else {
          bool dup = false;
          for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t e = base + lane;
            const bool val = e < len;
            const uint32_t efo = val ? l_ol[e] & 0xFFFFu : 0;
            const uint64_t md = __ballot(val && efo == fo), mb = __ballot(val && efo > fo);
            if (md | mb) {
              const int f = __builtin_ctzll(md | mb);
              if ((md >> f) & 1)
                dup = true;  // an equal offset: `in` is not listed
              else
                pos = (int)(base + f);
              break;
            }
          }
          if (!dup && pos < 0) pos = (int)len;
        }
        if (pos >= 0) {
          // move [pos, len) up by one, from the tail
          for (uint32_t hi = len; hi > (uint32_t)pos;) {
            const uint32_t lo = hi - (uint32_t)pos > 64 ? hi - 64 : (uint32_t)pos;
            const uint32_t e = lo + lane;
            const bool val = e < hi && e + 1 < (uint32_t)CAP;
            const uint32_t vp = val ? l_pos[e] : 0, vo = val ? l_ol[e] : 0;
            __syncthreads();
            if (val) {
              l_pos[e + 1] = vp;
              l_ol[e + 1] = vo;
            }
            __syncthreads();
            hi = lo;
          }
          if (lane == 0 && (uint32_t)pos < (uint32_t)CAP) {
            l_pos[pos] = e_pos;
            l_ol[pos] = e_ol;
          }
          if (len < (uint32_t)CAP) len++;  // distinct 13-bit offsets: never more than 8192
          __syncthreads();
          if (len == 1 || (uint32_t)pos <= stop + 1) {
            // entries before the predecessor keep their links; find the first stop from there
            for (uint32_t base = pos > 0 ? (uint32_t)pos - 1 : 0; base < len; base += 64) {
              const uint32_t e = base + lane;
              const bool val = e < len;
              const uint32_t p = val ? l_pos[e] : 0, ol = val ? l_ol[e] : 0;
              const uint32_t nx = val && e + 1 < len ? l_ol[e + 1] & 0xFFFFu : 0xFFFFFFFFu;
              const bool st = val && (!(p & kMore) || (((ol & 0xFFFFu) + (ol >> 16)) & 0xFFFFu) != nx);  // :138-146
              const uint64_t m = __ballot(st);
              if (m) {
                stop = base + (uint32_t)__builtin_ctzll(m);
                break;
              }
            }
            complete = (l_ol[0] & 0xFFFFu) == 0 && !(l_pos[stop] & kMore);  // :133, :138
            fresh = false;
          }
        }
        const bool carried = tp < a.carry;
        const bool emit = T > 0 && complete && !carried;
        if (emit && !fresh) {  // the payload's bytes from the head through `stop`, and the head (:155-175)
          uint32_t sum = 0;
          for (uint32_t e = lane; e <= stop; e += 64) sum += a.w.info[a.perm[s + (l_pos[e] & kPosMask)]].z;
          for (int m = 32; m; m >>= 1) sum += (uint32_t)__shfl_xor((int)sum, m);
          c_pay = sum;
          c_head = a.perm[s + (l_pos[0] & kPosMask)];
          c_hdr = a.w.info[c_head].w + 40;
          fresh = true;
        }
        if (lane == t) {
          my_v = carried ? GPK_DEFRAG6_CARRIED : emit ? 0 : GPK_DEFRAG6_HELD;
          my_listed = pos >= 0;
          if (emit) {
            my_size = c_hdr + c_pay;
            my_pay = c_pay;
            my_head = c_head;
          }
        }
      }
      if (lane < cnt) {
        a.verdict[pkt] = my_v;
        a.w.listed[pkt] = my_listed;
        if (my_size) {
          a.w.dsize[pkt] = my_size;
          a.w.dpay[pkt] = my_pay;
          a.w.dhead[pkt] = my_head;
        }
      }
    }
    // perm is ascending inside a key, so "arrived by packet i" is "index <= i"
    for (uint32_t e = lane; e < len && e < k; e += 64) a.w.fin[s + e] = a.perm[s + (l_pos[e] & kPosMask)];
    if (lane == 0) a.w.fin_len[g] = len < k ? len : k;
    __syncthreads();
  }
}

using DnumIt = hipcub::TransformInputIterator<uint32_t, NonZero, const uint32_t*>;
using DdstIt = hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*>;

__global__ void __launch_bounds__(256) finish6_kernel(const int32_t* group_of, const uint32_t* start, uint64_t n, Work w,
                                                      gpk_datagrams6 o) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = group_of[i];
  if (g < 0) o.verdict[i] = g;
  const uint32_t sz = w.dsize[i], j = w.dnum[i];
  const uint64_t at = w.ddst[i];
  if (sz) {
    o.verdict[i] = (int32_t)j;
    o.last[j] = (uint32_t)i;
    o.head[j] = w.dhead[i];
    o.length[j] = w.dpay[i];
    o.offsets[j] = at;
    o.caplens[j] = sz;
    o.payload_off[j] = sz - w.dpay[i];
    w.desc[2 * (uint64_t)j] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), sz, sz - w.dpay[i]);
    w.desc[2 * (uint64_t)j + 1] = make_uint4(start[g], w.fin_len[g], (uint32_t)i, w.dhead[i]);
  }
  const uint32_t p = w.listed[i];
  if (p) o.pending[w.ppos[i]] = (uint32_t)i;
  if (i + 1 == n) {
    o.counts[0] = j + (sz != 0);
    o.counts[1] = w.ppos[i] + p;
    o.counts[2] = at + sz;
    o.counts[3] = at + sz > o.data_cap;
  }
}

// ---- time: the deferred stamp (defrag.go:84-87) and DiscardOlderThan (:183-194)
struct TimeWork {
  int64_t* key_seen;  // [n] per group: the key's time
  uint32_t* dead;     // [n] per group: discarded
};

__global__ void __launch_bounds__(256) key6_kernel(const uint32_t* perm, const uint32_t* start, const uint32_t* gcounts,
                                                   uint64_t n, TimeWork tw, gpk_defrag6_time tm) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t dead = 0;
  if (g < n && g < gcounts[0]) {
    // perm is ascending inside a key and every call stamps: the key's last packet made the last stamp
    const int64_t ks = tm.seen[perm[start[g + 1] - 1]];
    dead = tm.discard && ks < tm.t;
    tw.key_seen[g] = ks;
    tw.dead[g] = dead;
  }
  const uint32_t keys = (uint32_t)__popcll(__ballot(dead != 0));
  if ((threadIdx.x & 63) == 0 && keys) atomicAdd((unsigned long long*)&tm.counts[0], (unsigned long long)keys);
}

__global__ void __launch_bounds__(256) drop6_kernel(const int32_t* group_of, uint64_t n, TimeWork tw, uint32_t* listed,
                                                    uint64_t* counts) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool drop = false;
  if (i < n) {
    const int32_t g = group_of[i];
    drop = g >= 0 && tw.dead[g] && listed[i];
    if (drop) listed[i] = 0;
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(drop));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd((unsigned long long*)&counts[1], (unsigned long long)c);
}

__global__ void __launch_bounds__(256) seen6_kernel(const int32_t* group_of, uint64_t n, const uint32_t* listed,
                                                    const uint32_t* ppos, TimeWork tw, int64_t* pending_seen) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (listed[i]) pending_seen[ppos[i]] = tw.key_seen[group_of[i]];  // listed: keyed
}

struct MoveArgs {
  const uint8_t* data;
  const uint64_t* offsets;
  Work w;
  const uint64_t* counts;
  uint8_t* out;
  uint64_t cap;
};

__global__ void __launch_bounds__(256) move6_kernel(MoveArgs a) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t D = a.counts[0];
  for (uint64_t j = blockIdx.x; j < D; j += gridDim.x) {
    const uint4 da = a.w.desc[2 * j], db = a.w.desc[2 * j + 1];
    const uint64_t at = (uint64_t)da.y << 32 | da.x;
    const uint32_t size = da.z, hdr = da.w, total = size - hdr;
    if (at + size > a.cap) continue;  // a datagram that does not fit is not written at all
    const uint32_t s = db.x, flen = db.y, last = db.z;
    uint8_t* dgram = a.out + at;
    // the list at the time of packet `last`: the final list's entries that had arrived by then
    uint32_t dst = 0, ord = 0, nh = 0;
    bool done = false;
    for (uint32_t base = 0; base < flen && !done; base += 64) {
      const uint32_t e = base + lane;
      const uint32_t pk = e < flen ? a.w.fin[s + e] : 0xFFFFFFFFu;
      const bool keep = pk <= last;
      uint4 inf = make_uint4(0, 0, 0, 0);
      uint64_t src = 0;
      if (keep) {
        inf = a.w.info[pk];
        src = a.offsets[pk] + inf.y;
      }
      for (uint64_t m = __ballot(keep); m; m &= m - 1) {
        const int b = __builtin_ctzll(m);
        const uint32_t plen = (uint32_t)__shfl((int)inf.z, b), x = (uint32_t)__shfl((int)inf.x, b);
        const uint64_t from = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(src >> 32), b) << 32 |
                              (uint32_t)__shfl((int)(uint32_t)src, b);
        if (plen > total - dst) {  // never: the plan summed these same lengths
          done = true;
          break;
        }
        if ((ord & 3u) == wave) gpk::copy_bytes(dgram + hdr + dst, a.data + from, plen, lane);
        dst += plen;
        ord++;
        if (!((x >> 16) & 1u)) {  // `more` unset: the last fragment, whose Next Header the result takes
          nh = x >> 24;
          done = true;
          break;
        }
      }
    }
    if (wave != 3) continue;
    // the header: the head packet from its start through the IPv6 header, with
    // Version 6, the payload's length and the last fragment's Next Header
    const uint8_t* hs = a.data + a.offsets[db.w];
    const uint32_t s6 = hdr - 40, plf = total > 0xFFFFu ? 0u : total;
    for (uint32_t b = lane; b < hdr; b += 64) {
      uint32_t v = hs[b];
      const uint32_t rel = b - s6;  // wraps for the bytes before the IPv6 header
      if (rel == 0) v = (v & 0x0Fu) | 0x60u;
      if (rel == 4) v = plf >> 8;
      if (rel == 5) v = plf & 0xFFu;
      if (rel == 6) v = nh;
      dgram[b] = (uint8_t)v;
    }
  }
}

}  // namespace

struct gpk_defragger6 {
  int device = 0;
  uint64_t cap = 0;
  Work w{};
  TimeWork tw{};
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  gpk::Workspace ws;
};

namespace {

void carve(gpk_defragger6* d) {  // every device array of the handle
  const uint64_t n = d->cap;
  d->ws.take(d->w.info, n), d->ws.take(d->w.desc, 2 * n), d->ws.take(d->w.listed, n), d->ws.take(d->w.dsize, n);
  d->ws.take(d->w.dpay, n), d->ws.take(d->w.dhead, n), d->ws.take(d->w.dnum, n), d->ws.take(d->w.ddst, n);
  d->ws.take(d->w.ppos, n), d->ws.take(d->w.fin, n), d->ws.take(d->w.fin_len, n), d->ws.take(d->tw.key_seen, n);
  d->ws.take(d->tw.dead, n), d->ws.take(d->tmp, d->tmp_bytes);
}

}  // namespace

extern "C" int gpk_defragger6_create(gpk_defragger6** out, int device, uint64_t max_packets) {
  if (const int rc = gpk::check_create(out, device, max_packets)) return rc;
  gpk::DeviceScope dscope(device);  // the caller's device is restored on return
  if (dscope.err != hipSuccess) return GPK_EHIP;
  gpk_defragger6* d = new (std::nothrow) gpk_defragger6();
  if (!d) return GPK_ENOMEM;
  d->device = device;
  d->cap = max_packets;
  const uint64_t n = max_packets;
  size_t b0 = 0, b1 = 0, b2 = 0;
  bool ok = hipcub::DeviceScan::ExclusiveSum(nullptr, b0, DnumIt(nullptr, NonZero()), (uint32_t*)nullptr, (int)n) ==
                hipSuccess &&
            hipcub::DeviceScan::ExclusiveSum(nullptr, b1, DdstIt(nullptr, Widen()), (uint64_t*)nullptr, (int)n) ==
                hipSuccess &&
            hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n) ==
                hipSuccess;
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

extern "C" int gpk_defragger6_destroy(gpk_defragger6* d) {
  if (!d) return GPK_EINVAL;
  gpk::DeviceScope dscope(d->device);
  (void)hipDeviceSynchronize();
  d->ws.release();
  delete d;
  return GPK_OK;
}

namespace {

// tm == nullptr: gpk_defrag6_batch
int defrag6_run(gpk_defragger6* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g, uint64_t carry,
                const gpk_datagrams6* o, const gpk_defrag6_time* tm, void* stream) {
  if (!d || !b || !r || !g || !o || !o->counts) return GPK_EINVAL;
  const uint64_t n = b->n;
  if (n > d->cap || carry > n) return GPK_EINVAL;
  if (n && (!b->data || !b->offsets || !r->layouts || !g->group_of || !g->perm || !g->start || !g->counts ||
            !o->verdict || !o->last || !o->head || !o->length || !o->offsets || !o->caplens || !o->payload_off ||
            !o->pending || (!o->data && o->data_cap)))
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
  hipLaunchKernelGGL(prep6_kernel, grd, blk, 0, s, b->data, b->offsets, r->layouts, g->group_of, n, w);
  // one wave per key, striding: at most n keys
  const unsigned pblocks = (unsigned)std::min<uint64_t>(n, 1u << 18);
  const PlanArgs pa{g->perm, g->start, g->counts, (uint32_t)carry, o->verdict, w};
  hipLaunchKernelGGL(plan6_kernel<kSmallCap>, dim3(pblocks), dim3(64), 0, s, pa);
  hipLaunchKernelGGL(plan6_kernel<GPK_DEFRAG6_MAX_LIST>, dim3(std::min(pblocks, 4096u)), dim3(64), 0, s, pa);
  if (tm) {
    hipLaunchKernelGGL(key6_kernel, grd, blk, 0, s, g->perm, g->start, g->counts, n, d->tw, *tm);
    if (tm->discard) hipLaunchKernelGGL(drop6_kernel, grd, blk, 0, s, g->group_of, n, d->tw, w.listed, tm->counts);
  }
  size_t tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, DnumIt(w.dsize, NonZero()), w.dnum, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, DdstIt(w.dsize, Widen()), w.ddst, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  tb = d->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(d->tmp, tb, (const uint32_t*)w.listed, w.ppos, (int)n, s) != hipSuccess)
    return GPK_EHIP;
  hipLaunchKernelGGL(finish6_kernel, grd, blk, 0, s, g->group_of, g->start, n, w, *o);
  if (tm) hipLaunchKernelGGL(seen6_kernel, grd, blk, 0, s, g->group_of, n, w.listed, w.ppos, d->tw, tm->pending_seen);
  // one block per datagram, striding: a packet returns at most one
  const MoveArgs ma{b->data, b->offsets, w, o->counts, o->data, o->data_cap};
  hipLaunchKernelGGL(move6_kernel, dim3((unsigned)std::min<uint64_t>(n, 65536)), blk, 0, s, ma);
  return hipGetLastError() == hipSuccess ? GPK_OK : GPK_EHIP;
}

}  // namespace

extern "C" int gpk_defrag6_batch(gpk_defragger6* d, const gpk_batch* b, const gpk_results* r, const gpk_groups* g,
                                 uint64_t carry, const gpk_datagrams6* o, void* stream) {
  return defrag6_run(d, b, r, g, carry, o, nullptr, stream);
}

extern "C" int gpk_defrag6_batch_timed(gpk_defragger6* d, const gpk_batch* b, const gpk_results* r,
                                       const gpk_groups* g, uint64_t carry, const gpk_datagrams6* o,
                                       const gpk_defrag6_time* tm, void* stream) {
  if (!tm) return GPK_EINVAL;
  return defrag6_run(d, b, r, g, carry, o, tm, stream);
}
