/*
 * gpk_defrag.h — IPv4 reassembly of a decoded batch on the device: what
 * ip4defrag's IPv4Defragmenter.DefragIPv4 does per packet (ip4defrag/defrag.go),
 * for a whole batch in HBM.
 *
 * A decoded batch (records + layouts) and its GPK_GROUP_DEFRAG grouping
 * (gpk_flows.h) go in. Out come the datagrams DefragIPv4 would have returned,
 * in the order it would have returned them, every packet's verdict, and the
 * fragments still waiting at the end of the batch. One call behaves like a fresh
 * NewIPv4Defragmenter() fed the batch's packets in batch order; the keyed
 * packets of a group are the calls that reach fragmentList.insert.
 *
 * Reproduced exactly, in uint16 arithmetic where Go uses uint16:
 *   insert (defrag.go:214-271)  fragOffset >= Highest pushes back; otherwise the
 *       list is scanned: an equal FragOffset is ignored (nil, nil) before any
 *       counter moves, else the fragment goes before the first larger offset; if
 *       there is none it is NOT listed but Highest/Current still move.
 *       fragLength = Length - 20 whatever the IHL. Highest and Current wrap.
 *   build (:276-326)            the overlap branch's currentOffset +=
 *       frag.FragOffset*8, "invalid fragment" and "hole found"; a failed build
 *       leaves the list as it was; a built datagram flushes the key.
 *   DefragIPv4WithTimestamp (:113-132)  out == nil && List.Len()+1 > 8192
 *       flushes the key and reports the "maximum size" error.
 *   frag.Payload[startAt:] with startAt > len(Payload) (a truncated capture)
 *       panics in Go: reported as GPK_DEFRAG_EPANIC, no datagram, the list and
 *       the counters as the insert left them. The maximum-length check is
 *       applied after it like after every other nil result, so at 8192 entries
 *       GPK_DEFRAG_EMAXLEN wins.
 *   Payload of a fragment is the decode's: data[IHL*4 : min(len(data), Length)]
 *       of the IPv4's slice, Length = uint16(len(data)) where the field is 0
 *       (ip4.go:189-214).
 *
 * Harness rule (as in gpk_flows.h): "the IPv4" of a packet is its layout
 * slot's last IPv4, the one the grouping keyed.
 *
 * Time (gpk_defrag_batch_timed): fragmentList.LastSeen and DiscardOlderThan
 * (:138-149). Timestamps are int64 nanoseconds (time.Time.UnixNano()), Before
 * is <.
 *   LastSeen = t (:249) is an assignment made by every call that passes the
 *       duplicate check: "counted, not listed" fragments and fragments whose
 *       build then fails stamp too; an ignored duplicate (:223-238) returns
 *       before it, and calls that fail the security checks never reach insert.
 *       `pending` lists exactly those stamping fragments of the live keys in
 *       arrival order, so a key's LastSeen is seen[] of its last pending packet.
 *   DiscardOlderThan(t) after the batch: keys with LastSeen < t leave pending.
 * gpk_defrag_batch itself keeps no time.
 *
 * Cost: the list walk of one key is done by one wave (64 list entries per
 * step); build is sequential in list order, so a key that re-builds on every
 * one of its k fragments costs O(k^2). That is a documented limit, not a target.
 */
#ifndef GPK_DEFRAG_H
#define GPK_DEFRAG_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"
#include "gpk_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* verdict[i] < 0 for a keyed packet (the grouping's GPK_GROUP_* codes are
 * carried over for the others) */
#define GPK_DEFRAG_HELD (-16)     /* (nil, nil): inserted, counted or ignored as a duplicate     */
#define GPK_DEFRAG_EHOLE (-17)    /* "defrag: building - hole found"              defrag.go:301 */
#define GPK_DEFRAG_EINVALID (-18) /* "defrag: building - invalid fragment"                  :293 */
#define GPK_DEFRAG_EMAXLEN (-19)  /* "Fragment List hits its maximum size"; key flushed     :118 */
#define GPK_DEFRAG_EPANIC (-20)   /* frag.Payload[startAt:] out of range: Go panics         :295 */

#define GPK_DEFRAG_MAX_LIST 8192  /* IPv4MaximumFragmentListLen */

typedef struct gpk_defragger gpk_defragger;

/* Workspace for batches of up to max_packets (< 2^28) on one device; it serves
 * one call at a time, like a grouper's. */
int gpk_defragger_create(gpk_defragger** out, int device, uint64_t max_packets);
int gpk_defragger_destroy(gpk_defragger* d);

/* Device arrays, caller-allocated, n = batch size. Datagrams are numbered in
 * the order of the packet that completed them (the order DefragIPv4 returned
 * them in); at most n/2 + 1 exist, arrays of n entries always suffice.
 *
 * data holds every datagram as: the bytes of `in` (the packet whose call
 * completed it) from the packet start through the end of its IPv4 header,
 * then the reassembled payload. In the copied IPv4 header flags and fragment
 * offset are 0, Total Length is IHL*4 + payload bytes (0 when that exceeds 16
 * bits: DecodeFromBytes then takes the slice's length, ip4.go:189-193) and the
 * header checksum is recomputed. So
 *   data[offsets[j] + payload_off[j] : offsets[j] + caplens[j]]  ==  out.Payload
 * and {data, offsets, caplens, counts[0]} is a gpk_batch the parsers decode:
 * IPv4, then UDP/TCP with the L4 checksum and flows over the whole datagram.
 * The IPv4.Length such a re-decode reports (header + payload) is not
 * out.Length: the reference stores Highest, the payload's length, there
 * (defrag.go:311); length[j] carries the reference's value.
 *
 * data_cap: the kernel never writes at or past data + data_cap. The sum of the
 * batch's caplens is always enough: a packet's payload enters at most one
 * datagram and `in` gives its header to at most one, both from inside its
 * caplen. A datagram that does not fit is not written at all; counts[3] is set
 * and counts[2] says how much is needed. */
typedef struct gpk_datagrams {
  int32_t* verdict;      /* [n]  >= 0: this packet completed datagram verdict[i]; else a
                                 GPK_DEFRAG_* or GPK_GROUP_* code                            */
  uint32_t* last;        /* [n]  `in`: the packet that completed datagram j                  */
  uint32_t* length;      /* [n]  out.Length = Highest                                        */
  uint64_t* offsets;     /* [n]  datagram j's bytes in data                                  */
  uint32_t* caplens;     /* [n]                                                              */
  uint32_t* payload_off; /* [n]  where out.Payload starts inside datagram j                  */
  uint32_t* pending;     /* [n]  ascending packet indices of every fragment whose insert
                                 reached the counter update, for keys not flushed by the end
                                 of the batch ("counted, not listed" ones included). These
                                 packets, in this order, in front of the next batch
                                 reproduce the reference's state                             */
  uint64_t* counts;      /* [4]  datagrams, pending packets, bytes of data needed, overflow  */
  uint8_t* data;         /* [data_cap]                                                       */
  uint64_t data_cap;
} gpk_datagrams;

/* Reassemble. batch, res (records + layouts) and groups (a GPK_GROUP_DEFRAG
 * grouping of this batch, by gpk_group_batch or gpk_decode_group_batch + a
 * decode with layouts) are device-resident. Asynchronous on `stream`. */
int gpk_defrag_batch(gpk_defragger* d, const gpk_batch* batch, const gpk_results* res, const gpk_groups* groups,
                     const gpk_datagrams* out, void* stream);

/* Time for gpk_defrag_batch_timed: device arrays, n = batch size. A live key
 * has been stamped at least once, so Go's zero time.Time never shows. */
typedef struct gpk_defrag_time {
  const int64_t* seen;   /* [n]  packet i's DefragIPv4WithTimestamp timestamp; for a fragment
                                 carried over from an earlier batch its key's LastSeen
                                 (pending_seen of that batch), which replays to the same state */
  uint32_t discard;      /*      != 0: DiscardOlderThan(t) runs after the batch                  */
  int64_t t;
  int64_t* pending_seen; /* [n]  out: LastSeen of pending[k]'s key                               */
  uint64_t* counts;      /* [2]  out: keys discarded (the reference's return value), packets
                                 dropped with them                                               */
} gpk_defrag_time;

/* gpk_defrag_batch, then the time operations: out->pending and out->counts[1]
 * hold the survivors of the discard. Everything else is gpk_defrag_batch's. */
int gpk_defrag_batch_timed(gpk_defragger* d, const gpk_batch* batch, const gpk_results* res, const gpk_groups* groups,
                           const gpk_datagrams* out, const gpk_defrag_time* tm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPK_DEFRAG_H */
