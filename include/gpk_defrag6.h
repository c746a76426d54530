/*
 * gpk_defrag6.h — IPv6 reassembly of a decoded batch on the device: what
 * ip6defrag's IPv6Defragmenter.DefragIPv6 does per packet (ip6defrag/defrag.go),
 * for a whole batch in HBM.
 *
 * A decoded batch (records + layouts) and its GPK_GROUP_DEFRAG6 grouping
 * (gpk_flows.h) go in. Out come the IPv6 layers DefragIPv6 would have returned,
 * in the order it would have returned them, every packet's verdict, and the
 * fragments it holds at the end of the batch. One call behaves like a fresh
 * NewIPv6Defragmenter() fed the batch's keyed packets in batch order.
 *
 * Reproduced exactly (defrag.go:82-178), per call DefragIPv6(ipv6, fg):
 *   - in = {fg.FragmentOffset, fg.LayerPayload(), fg.MoreFragments,
 *     fg.NextHeader}; in.ipv6 = ipv6 only at offset 0. The key is
 *     fg.Identification alone: addresses do not enter it.
 *   - the first call for an Identification stores `in` and returns nil, even
 *     when that fragment is whole on its own (offset 0, M = 0)          :98-103
 *   - otherwise the list is scanned from its head: an entry with an equal
 *     offset ends the scan and `in` is NOT listed (the first arrival wins,
 *     whatever its bytes); else `in` goes before the first larger offset; else
 *     it is appended. The list is strictly ascending: at most 8192 entries
 *     (the offset has 13 bits)                                         :107-129
 *   - a head whose offset is not 0 returns nil                         :133-135
 *   - the walk from the head goes on while `more` is set and needs
 *     f.offset + uint16(len(f.payload)/8) == f.next.offset, in uint16
 *     arithmetic with a floor division; the first entry with `more` unset
 *     ends it with success; entries behind that entry are never read   :137-152
 *   - the result's Payload is the concatenation from the head through that
 *     entry, NextHeader is that LAST entry's, TrafficClass, FlowLabel,
 *     HopLimit, SrcIP and DstIP are the head's ipv6's, Version is the constant
 *     6 and Length stays 0                                             :155-177
 *   - nothing is ever removed: a key is never flushed, so a completed
 *     datagram is returned again by every later call on its key (a duplicate,
 *     a fragment behind the final one), and completeness is not monotone (a
 *     fragment inserted into a complete chain can break it).
 *
 * Harness rules (the reference leaves them to its caller; fixed here as in
 * gpk_flows.h and gpk_defrag.h):
 *   - "the IPv6" of a packet is its layout slot's last IPv6 (GPK_DEC_IPV6). The
 *     packet is considered when that slot is present, whatever a later layer
 *     returned, and whether or not GPK_DEC_IPV6_EXT is registered.
 *   - "the fragment header" is found by a walk of its own: from the
 *     LayerPayload() and next header IPv6.DecodeFromBytes left (ip6.go:235-275:
 *     an inline HopByHop already consumed, a jumbogram's payload starting at
 *     its HopByHop header, trimmed to Length), headers 0, 43 and 60 are skipped
 *     as decodeIPv6ExtensionBase reads them ((b[1]+1)*8, ip6.go:418-432); fewer
 *     than 2 bytes, or fewer than the stated length, stop the walk unkeyed; it
 *     ends at the first next-header 44 with at least 8 bytes there. Any other
 *     next header: GPK_GROUP_NONE.
 *   - fg is what decodeIPv6Fragment reads from those 8 bytes (ip6.go:648-661):
 *     NextHeader b[0], FragmentOffset BE16(b[2:4])>>3, MoreFragments b[3]&1,
 *     Identification BE32(b[4:8]); fg.LayerPayload() is the rest of that IPv6
 *     payload as captured (a truncated capture gives fewer bytes).
 *   - every call gets an IPv6 value of its own, as NewPacket gives the
 *     documented caller (defrag.go:63-81): a datagram's header fields are those
 *     of the listed offset-0 fragment's packet.
 *   - the example's "ignore unless UDP or TCP" filter is the caller's and is
 *     not applied.
 *
 * Time (gpk_defrag6_batch_timed): the entry's time and DiscardOlderThan
 * (:183-194). Timestamps are int64 nanoseconds (time.Time.UnixNano()), Before
 * is <.
 *   - the deferred d.container[fg.Identification].time = time.Now() (:84-87)
 *     runs after EVERY call on the Identification and stamps the key's head
 *     entry as it is then: the first call, ignored duplicates and calls that
 *     return a datagram included. DiscardOlderThan reads the head entry's time
 *     too, and a head replaced by an insert in front of it is stamped by that
 *     very call, so a key's time is the timestamp of its last call.
 *   - scope decision: the reference has no timestamp parameter here and reads
 *     the wall clock. The caller's timestamp plays time.Now(), as
 *     DefragIPv4WithTimestamp's does for IPv4.
 *   - `carry` packets stamp too; their seen[] is the carried key time, so a
 *     replay reproduces it even when the last stamper was an unlisted duplicate.
 *   - DiscardOlderThan(t) after the batch: keys with time < t leave pending.
 * gpk_defrag6_batch itself keeps no time; without a discard the reference
 * removes nothing, and a caller that wants state to shrink otherwise drops
 * pending packets itself (gopacket_amd.flows.IPv6Defragmenter: flush,
 * drop_completed).
 *
 * Cost: one wave per key walks its packets; a lookup or insert touches the list
 * 64 entries at a time. The position of the first stop of the head's chain is
 * kept, so an in-order fragment and a call after completion cost O(1) list
 * steps; an insert in front of that position rescans from its predecessor. The
 * byte mover derives a datagram's fragments from the key's final list, filtered
 * by arrival, so re-emission costs no quadratic segment lists.
 */
#ifndef GPK_DEFRAG6_H
#define GPK_DEFRAG6_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"
#include "gpk_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* verdict[i] < 0 for a keyed packet (the grouping's GPK_GROUP_* codes are
 * carried over for the others) */
#define GPK_DEFRAG6_HELD (-32)    /* nil: stored, listed or ignored as a duplicate, nothing returned */
#define GPK_DEFRAG6_CARRIED (-33) /* one of the `carry` leading packets: state only               */

#define GPK_DEFRAG6_MAX_LIST 8192 /* distinct 13-bit offsets */

typedef struct gpk_defragger6 gpk_defragger6;

/* Workspace for batches of up to max_packets (< 2^28) on one device; it serves
 * one call at a time, like a grouper's. */
int gpk_defragger6_create(gpk_defragger6** out, int device, uint64_t max_packets);
int gpk_defragger6_destroy(gpk_defragger6* d);

/* Device arrays, caller-allocated, n = batch size. Datagrams are numbered in
 * the order of the packets whose calls returned them; a packet returns at most
 * one, so arrays of n entries always suffice.
 *
 * data holds every datagram as: the HEAD packet's bytes (the listed offset-0
 * fragment's) from the packet start through its 40-byte IPv6 header, then the
 * reassembled payload. In the copied IPv6 header the version nibble is written
 * as 6, Payload Length is the payload's byte count (0 when that exceeds 65535:
 * a re-decode then reports the reference's own zero-length error) and Next
 * Header is the last fragment's; everything else is verbatim. Extension headers
 * in front of the Fragment header are dropped, as the reference's result has
 * none. So
 *   data[offsets[j] + payload_off[j] : offsets[j] + caplens[j]]  ==  l.Payload
 * and {data, offsets, caplens, counts[0]} is a gpk_batch the parsers decode.
 * The reference's own l.Length is 0; length[j] is len(l.Payload), also past
 * 65535.
 *
 * data_cap: the kernel never writes at or past data + data_cap. UNLIKE IPv4
 * (gpk_defrag.h) the sum of the batch's caplens is NOT a bound: a key is never
 * flushed, so every later call on a completed key returns its datagram again
 * and the same payload bytes enter many datagrams. A datagram that does not fit
 * is not written at all; counts[3] is set and counts[2] says how much is
 * needed, so a caller sizes data from a first call or retries. */
typedef struct gpk_datagrams6 {
  int32_t* verdict;      /* [n]  >= 0: this packet's call returned datagram verdict[i]; else
                                 GPK_DEFRAG6_HELD, GPK_DEFRAG6_CARRIED or a GPK_GROUP_* code */
  uint32_t* last;        /* [n]  the packet whose call returned datagram j                   */
  uint32_t* head;        /* [n]  the packet that gave its header: the listed offset-0 one     */
  uint32_t* length;      /* [n]  len(l.Payload); the reference's l.Length is 0                */
  uint64_t* offsets;     /* [n]  datagram j's bytes in data                                  */
  uint32_t* caplens;     /* [n]                                                              */
  uint32_t* payload_off; /* [n]  where l.Payload starts inside datagram j                    */
  uint32_t* pending;     /* [n]  ascending packet indices of every LISTED fragment (ignored
                                 duplicates are not in it). These packets, in this order, as
                                 the `carry` leading packets of the next batch reproduce the
                                 reference's state: first arrivals stay first, and nothing
                                 was ever removed                                            */
  uint64_t* counts;      /* [4]  datagrams, pending packets, bytes of data needed, overflow  */
  uint8_t* data;         /* [data_cap]                                                       */
  uint64_t data_cap;
} gpk_datagrams6;

/* Reassemble. batch, res (records + layouts) and groups (the GPK_GROUP_DEFRAG6
 * grouping of this batch by gpk_group_batch) are device-resident. The calls of
 * the first `carry` packets build state only: their verdict is
 * GPK_DEFRAG6_CARRIED, and a datagram they would have returned is neither
 * emitted nor numbered (without it, replaying the pending packets would return
 * datagrams a second time). Asynchronous on `stream`. */
int gpk_defrag6_batch(gpk_defragger6* d, const gpk_batch* batch, const gpk_results* res, const gpk_groups* groups,
                      uint64_t carry, const gpk_datagrams6* out, void* stream);

/* Time for gpk_defrag6_batch_timed: device arrays, n = batch size. Every key
 * has been stamped by its first call, so Go's zero time.Time never shows. */
typedef struct gpk_defrag6_time {
  const int64_t* seen;   /* [n]  the timestamp of packet i's call; for a `carry` packet its key's
                                 time (pending_seen of the batch it comes from)                  */
  uint32_t discard;      /*      != 0: DiscardOlderThan(t) runs after the batch                  */
  int64_t t;
  int64_t* pending_seen; /* [n]  out: the time of pending[k]'s key                               */
  uint64_t* counts;      /* [2]  out: keys discarded (the reference's return value), listed
                                 fragments dropped with them                                     */
} gpk_defrag6_time;

/* gpk_defrag6_batch, then the time operations: out->pending and
 * out->counts[1] hold the survivors of the discard. Everything else is
 * gpk_defrag6_batch's. */
int gpk_defrag6_batch_timed(gpk_defragger6* d, const gpk_batch* batch, const gpk_results* res,
                            const gpk_groups* groups, uint64_t carry, const gpk_datagrams6* out,
                            const gpk_defrag6_time* tm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPK_DEFRAG6_H */
