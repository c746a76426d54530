/*
 * gpk_tcpasm.h — TCP stream reassembly of a decoded batch on the device: what
 * tcpassembly's Assembler.AssembleWithTimestamp does per packet
 * (tcpassembly/assembly.go), for a whole batch in HBM.
 *
 * A decoded batch (records + layouts) and its GPK_GROUP_CONNECTION grouping
 * (gpk_flows.h) go in. Out come the Reassembly objects every stream would have
 * been handed, in order, with Skip/Start/End; every stream's bytes laid out
 * contiguously; every packet's verdict; and the state that lets the next batch
 * continue. One call behaves like a fresh NewAssembler(NewStreamPool(factory))
 * with MaxBufferedPagesPerConnection = max_pages (0 = unlimited) and
 * MaxBufferedPagesTotal = 0, fed the keyed packets of the batch in batch order,
 * followed by FlushAll() if `flush` is set.
 *
 * Reproduced exactly:
 *   Sequence.Difference (assembly.go:57-64)  int64, the quarter-space wrap rule
 *       as written. It is no total order: every comparison is the reference's,
 *       in the reference's scan direction. Add masks to 32 bits; invalid = -1.
 *   lookup (:552-566)  a bare FIN/RST (!SYN, empty payload) on a key with no
 *       open connection creates nothing: GPK_TCPASM_NOCONN. Otherwise a missing
 *       connection is created: a new stream instance (one factory.New). A key
 *       is directional; a key closed earlier in the batch gets a new instance.
 *   first SYN while nextSeq is invalid (:571-582)  a chunk with Start, the whole
 *       payload, nextSeq = seq + len + 1. End is NOT set on it.
 *   byteSpan (:612-623)  overlap trimming, and len(bytes) < span: empty bytes,
 *       nextSeq unchanged (a retransmitted SYN or an old retransmission
 *       delivers an empty chunk). End = RST || FIN also on such a chunk.
 *   sendToConnection (:627-636)  addContiguous pops every first page with
 *       Difference(nextSeq, first.seq) <= 0; the connection closes only if the
 *       LAST chunk of the call has End; closing drops the remaining pages.
 *   insertIntoConn (:686-759)  pages of 1900 bytes, an empty payload makes one,
 *       only the last page carries End; the chain goes in whole after the first
 *       entry met scanning from the back for which prev.seq.Difference(seq) < 0
 *       is false; with max_pages > 0 and pages >= max_pages after the insert
 *       ONE page is popped, and sendToConnection follows.
 *   addNextFromConn (:763-783)  Skip = -1 while nextSeq is invalid, the
 *       difference when it is > 0 (it can exceed 2^31: int64), else 0.
 *   FlushAll (:279-290)  per open connection skipFlush until closed; each
 *       repetition is one Reassembled call, the last one only closes.
 *   panic("wtf") (:716-718)  first.seq == nextSeq at an insert. No traffic
 *       reaches it (such a page is always popped before nextSeq rests); a
 *       carried state can state it: GPK_TCPASM_EPANIC, connection left as it was.
 *
 * Harness rules (as in gpk_flows.h): "the TCP" of a packet is its layout
 * slot's last TCP, the one the grouping keyed; its payload is the
 * (layout.end[TCP] - start) - DataOffset*4 bytes after the header (none where
 * the header claims more than the slice holds).
 *
 * Time (gpk_tcpasm_batch_timed): lastSeen, page.Seen and FlushWithOptions{T}
 * (FlushOlderThan). Timestamps are int64 nanoseconds (time.Time.UnixNano()),
 * Before is <; Go's zero time.Time (a fresh lastSeen) is INT64_MIN, so callers'
 * timestamps must be greater than INT64_MIN.
 *   lastSeen (:567-569)  every call that gets a connection does
 *       if lastSeen.Before(ts) lastSeen = ts: a maximum, not the last value.
 *       "Useless" packets (:538) and GPK_TCPASM_NOCONN calls never reach it.
 *   A connection created in the batch starts from INT64_MIN. SCOPE DECISION that
 *       departs from the reference: connection.reset (:388-396) does not clear
 *       lastSeen and StreamPool recycles connection structs from a LIFO free
 *       list (:479-493, :662-667), so in the reference a new connection inherits
 *       the lastSeen of whatever closed connection last used its struct: a
 *       serial dependency across all keys. It shows only when timestamps run
 *       backwards (a new connection's first packet otherwise overwrites it).
 *       The device starts every new connection fresh.
 *   page.Seen  the timestamp of the page's source packet; all pages of one
 *       packet share it. Reassembly.Seen of a chunk is seen[chunk.src].
 *   FlushWithOptions (:238-269) after the batch, per open connection: while the
 *       list is not empty and the FIRST page's Seen < T, skipFlush (round r is
 *       call GPK_TCPASM_CALL_FLUSH | r) — the contiguous pages behind that page
 *       go out whatever their age, and a young first page shields older pages
 *       behind it; a send whose last chunk has End closes the connection and
 *       ends the loop. With CloseAll a connection still open with an empty list
 *       and lastSeen < T is closed (call CALL_FLUSH | r). The reference visits
 *       the connections in a Go map's order, which is undefined: outputs stay
 *       stream-major.
 * gpk_tcpasm_batch itself keeps no time: a chunk names its source packet, so a
 * caller reads Seen from its own capture info. MaxBufferedPagesTotal is 0
 * always.
 *
 * Cost: one wave walks one key. In-order runs retire 64 packets per step; a
 * queued packet costs one back-scan of the key's page list (64 entries per
 * step) and a parallel shift. A key that inserts k pages at the front of a
 * list of k costs O(k^2 / 64).
 */
#ifndef GPK_TCPASM_H
#define GPK_TCPASM_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"
#include "gpk_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* verdict[i] of a keyed packet (the grouping's GPK_GROUP_* codes are carried
 * over for the others) */
#define GPK_TCPASM_DIRECT (-24)    /* delivered by its own Assemble call                      :571-605 */
#define GPK_TCPASM_QUEUED (-25)    /* insertIntoConn: cut into pages                              :715 */
#define GPK_TCPASM_NOCONN (-26)    /* bare FIN/RST, no open connection: nothing happens          :555 */
#define GPK_TCPASM_CARRIED (-27)   /* a carried entry (below), accepted                                */
#define GPK_TCPASM_EBADCARRY (-28) /* a carried entry that fits no carried connection: ignored         */
#define GPK_TCPASM_EPANIC (-29)    /* panic("wtf"): connection left as it was                    :717 */

#define GPK_TCPASM_PAGE_BYTES 1900 /* pageBytes */

/* gpk_tcp_chunk.flags */
#define GPK_TCP_START 1u
#define GPK_TCP_END 2u

/* gpk_tcp_chunk.call / stream_closed: GPK_TCPASM_CALL_FLUSH | round for the
 * connection's round-th skipFlush of FlushAll; stream_closed of an open stream */
#define GPK_TCPASM_CALL_FLUSH 0x80000000u
#define GPK_TCPASM_OPEN 0xFFFFFFFFu

/* conn_seq[g]: no connection is open for the key; -1 is open with an invalid nextSeq */
#define GPK_TCPASM_NO_CONN (-2)

/* opts.carry_code[i] */
#define GPK_TCPASM_CARRY_CONN 0x80000000u /* packet i names a key whose connection is open, nextSeq = carry_seq[i] */
#define GPK_TCPASM_CARRY_PAGE 0x40000000u /* | k: page k of packet i is listed on its connection                  */

typedef struct gpk_tcpasm gpk_tcpasm;

/* Workspace for batches of up to max_packets (< 2^28) on one device; it serves
 * one call at a time, like a grouper's. The page and chunk workspaces hold
 * n + data_bytes / 1900 entries and grow (a synchronising reallocation) in the
 * first call that needs more than any before it. */
int gpk_tcpasm_create(gpk_tcpasm** out, int device, uint64_t max_packets);
int gpk_tcpasm_destroy(gpk_tcpasm* a);

/* Streaming: the first `carried` packets of the batch are carried entries, not
 * traffic; they make no Assemble call.
 *   CARRY_CONN      the packet only names its key: the key's connection is open
 *                   at the start, nextSeq = carry_seq[i] (-1: invalid). It
 *                   counts as a stream instance created by that packet.
 *   CARRY_PAGE | k  page k of the packet is on its connection's list, behind the
 *                   entries carried before it; no limit check, no sorting. A
 *                   packet is repeated once per carried page (gpk_pack_batch
 *                   accepts repeated indices). A chunk popped from it names the
 *                   carried packet as src.
 * A CARRY_PAGE whose key has no CARRY_CONN before it, a second CARRY_CONN of a
 * key, or a page number the packet does not have: GPK_TCPASM_EBADCARRY, ignored.
 * conn_seq / first[g] / pend_* of one call, fed back this way in front of the
 * next batch, reproduce the reference's state. */
typedef struct gpk_tcpasm_opts {
  uint32_t max_pages;         /* MaxBufferedPagesPerConnection; 0 = unlimited */
  uint32_t flush;             /* FlushAll() after the batch                   */
  uint64_t carried;           /* 0 for a plain batch                          */
  const uint32_t* carry_code; /* [carried] device; NULL if carried == 0       */
  const int64_t* carry_seq;   /* [carried] device; read for CARRY_CONN        */
} gpk_tcpasm_opts;

/* One Reassembly. Consecutive chunks of a stream with equal `call` are one
 * Reassembled call. */
typedef struct gpk_tcp_chunk {
  uint64_t dst;     /*  0  where its bytes start in data                                     */
  int64_t skip;     /*  8  Reassembly.Skip                                                   */
  uint32_t src;     /* 16  the packet its bytes come from                                    */
  uint32_t src_off; /* 20  offset into that packet's TCP payload: 1900 * page + byteSpan's cut;
                           an emptied chunk points behind what was cut                       */
  uint32_t len;     /* 24  len(Bytes)                                                        */
  uint32_t call;    /* 28  the packet whose Assemble call delivered it, or CALL_FLUSH | round */
  uint32_t stream;  /* 32  its stream instance                                               */
  uint32_t flags;   /* 36  GPK_TCP_START, GPK_TCP_END                                        */
} gpk_tcp_chunk;

/* Device arrays, caller-allocated; n = batch size. Stream instances are
 * numbered in the order of their factory.New calls, i.e. by creating packet;
 * at most n exist. Chunks are stored stream-major: stream 0's in delivery
 * order, then stream 1's. Each ordinary packet yields at most
 * max(1, ceil(payload / 1900)) chunks and each carried entry at most one, so
 * chunk_cap = n + data_bytes / 1900 always suffices; the sum of the caplens
 * always suffices for data_cap. Nothing is written at or past either cap:
 * chunks that do not fit are dropped and counted; a stream whose bytes do not
 * fit is not written at all (its chunk table still is). counts says how much is
 * needed. */
typedef struct gpk_tcp_streams {
  int32_t* verdict;        /* [n]   GPK_TCPASM_* or GPK_GROUP_* code                            */
  int32_t* stream_of;      /* [n]   the instance the packet was routed to, or -1                */
  gpk_tcp_chunk* chunks;   /* [chunk_cap]                                                       */
  uint32_t* stream_group;  /* [n]   the stream's key (group id)                                 */
  uint32_t* stream_first;  /* [n]   the packet that created it                                  */
  uint32_t* stream_closed; /* [n]   `call` code of ReassemblyComplete, or GPK_TCPASM_OPEN       */
  uint32_t* stream_chunk0; /* [n+1] stream j's chunks are [stream_chunk0[j], stream_chunk0[j+1]) */
  uint64_t* stream_data0;  /* [n+1] stream j's bytes are data[stream_data0[j] : stream_data0[j+1]]:
                                    the concatenation of its chunks' bytes, what a
                                    tcpreader.ReaderStream without LossErrors would Read         */
  int64_t* conn_seq;       /* [n]   per group: GPK_TCPASM_NO_CONN, -1, or nextSeq at the end    */
  int32_t* conn_stream;    /* [n]   per group: the open connection's stream, or -1              */
  uint32_t* pend_pkt;      /* [chunk_cap] pages still listed: by group, then in list order      */
  uint32_t* pend_page;     /* [chunk_cap]   page number inside pend_pkt                         */
  uint64_t* counts;        /* [8]   streams, chunks, data bytes needed, pending pages, open
                                    connections, chunks dropped, data overflow (0/1); [7] is 0,
                                    or 1 where the batch's packets share bytes (the sum of the
                                    payloads exceeds data_bytes, which sizes the workspaces):
                                    nothing is assembled then and every other count is 0        */
  uint8_t* data;           /* [data_cap]                                                        */
  uint64_t chunk_cap;      /* bounds chunks, pend_pkt and pend_page                             */
  uint64_t data_cap;
} gpk_tcp_streams;

/* Reassemble. batch, res (records + layouts) and groups (a GPK_GROUP_CONNECTION
 * grouping of this batch) are device-resident. Asynchronous on `stream`. */
int gpk_tcpasm_batch(gpk_tcpasm* a, const gpk_batch* batch, const gpk_results* res, const gpk_groups* groups,
                     const gpk_tcpasm_opts* opts, const gpk_tcp_streams* out, void* stream);

/* Time for gpk_tcpasm_batch_timed. */
typedef struct gpk_tcpasm_time {
  const int64_t* seen;     /* [n] device: packet i's AssembleWithTimestamp timestamp; for a CARRY_CONN
                              entry the connection's lastSeen, for a CARRY_PAGE entry that page's Seen */
  uint32_t flush_older;    /* after the batch: 0 nothing, 1 FlushWithOptions{T}, 2 FlushWithOptions{T, CloseAll}
                              (= FlushOlderThan(T)); together with opts.flush: an argument error */
  int64_t t;
  int64_t* conn_last_seen; /* [n] out, per group: lastSeen of the connection open at the end
                              (INT64_MIN where none is)                                            */
  uint64_t* counts;        /* [2] out: flushed, closed: FlushWithOptions' two return values        */
} gpk_tcpasm_time;

/* gpk_tcpasm_batch with time. conn_last_seen[g] and seen[] of the pending
 * pages' packets, fed back as the seen[] of the next batch's carried entries,
 * reproduce the reference's state. */
int gpk_tcpasm_batch_timed(gpk_tcpasm* a, const gpk_batch* batch, const gpk_results* res, const gpk_groups* groups,
                           const gpk_tcpasm_opts* opts, const gpk_tcp_streams* out, const gpk_tcpasm_time* tm,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPK_TCPASM_H */
