/*
 * gpk_dns_streams.h — decode the DNS messages of reassembled TCP streams on the
 * device: gpk_tcpasm_batch (gpk_tcpasm.h) lays every stream's
 * bytes out contiguously, gpk_dns_rules.h decodes a DNS message from a buffer;
 * this entry group is the step between them. It finds the message boundaries
 * of every stream (RFC 1035 4.2.2: two length bytes in front of every
 * message), keeps an unfinished message across calls and runs
 * DNS.DecodeFromBytes (layers/dns.go:333-421) on each whole message.
 *
 * The reference has no such entry. The result is defined as what this Go
 * program on top of tcpassembly produces for one stream instance (one
 * direction), over the bytes its Reassembled calls deliver in order:
 *     read 2 bytes, big-endian Length; read Length more bytes;
 *     msg := make([]byte, Length) holding exactly those bytes;
 *     (&layers.DNS{}).DecodeFromBytes(msg, gopacket.NilDecodeFeedback)
 * Every message is one DecodeFromBytes call on a buffer of exactly its own
 * bytes, so every entry is something gpk_dns.h already defines (line numbers
 * as there: dns.go). The per-packet pass (gpk_dns.h, Slice) decodes the two
 * length bytes of a TCP payload as the ID, as the reference does; this pass
 * is the one that gives a DNS-over-TCP message as it was sent.
 *
 * Rules
 *   Message     A whole message gives a gpk_dns record, its gpk_dns_rr entries
 *               and its names. A message that fails on its own is a failed
 *               entry with the reference's error and arguments: every
 *               gpk_dns_err can occur. Length < 12 gives "DNS packet too
 *               short" (:338) with Truncated; Length == 0 decodes an empty
 *               buffer (the same error). Framing goes on behind a failed
 *               message: its length is known. The buffer ends with the
 *               message: a compression pointer cannot reach the previous or
 *               the next message (decodeName's checks are against len(data),
 *               :817,:844,:877-881).
 *   Offsets     hdr_off, data_off and the v[] offsets of gpk_dns_rr are relative
 *               to the stream's logical buffer (the carried tail, then this
 *               call's bytes). The message starts at hdr_off, behind its two
 *               length bytes.
 *   No magic    The framing has nothing to check: any two bytes are a length.
 *               There is no "not DNS" state; a stream of other bytes yields
 *               failed messages.
 *   Loss        A chunk with Skip > 0 ends the stream as GPK_DNSS_LOST. The
 *               bytes in front of the gap are framed. Nothing behind the gap
 *               is decoded.
 *   Close       stream_closed != GPK_TCPASM_OPEN gives GPK_DNSS_CLOSED. A loss
 *               wins over a close.
 *   Partial     An unfinished message in front of a loss or a close: the Go
 *               program's io.ReadFull fails and nothing is decoded. It gives
 *               one last entry with status GPK_DNSS_MSG_PARTIAL, err 0 and no
 *               entries; len is the prefix's Length (0 when fewer than 2
 *               bytes were there) and present the bytes that were there,
 *               counted from the prefix's first byte. DEPARTURE from
 *               gpk_tls_streams.h, which reports DecodeFromBytes(tail) there:
 *               TLS has a reference error for a short buffer that names what
 *               happened ("TLS packet length mismatch"); here the call would
 *               decode the front of a message as if it were whole and report
 *               an error of the noise behind the cut.
 *   No start    A chunk with Skip == -1 (no SYN seen) gives GPK_DNSS_NOSTART and
 *               no entries. With GPK_DNSS_FRAME_UNSTARTED such a stream is
 *               framed from its first byte instead.
 *   Synced      Otherwise the stream stays GPK_DNSS_SYNCED and its unfinished
 *               tail (one byte of a prefix, or a prefix and a part of the
 *               message) is copied to the tail arena, to be handed back in
 *               front of the stream's bytes of the next call: the tail arena
 *               of one call is the in->tails of the next. Length is 16 bits: a
 *               tail is at most 2 + 65535 - 1 = GPK_DNSS_MAX_TAIL bytes.
 *   Candidates  A stream is decoded when the TCP header of its creating packet
 *               (stream_first[j]) leads to LayerTypeDNS (107):
 *               TCP.NextLayerType() as tcp.go:591-597 writes it, destination
 *               port first, then source, looked up in the parser's tables, so
 *               RegisterTCPPortLayerType(5353, LayerTypeDNS) counts and port 53
 *               unregistered does not. The payload may be empty (a SYN has
 *               none). The server-to-client direction is a candidate too.
 *               Other streams get GPK_DNSS_NONE.
 *   Carried     in->state[j] other than NEW or SYNCED is final: the stream
 *               keeps it, nothing of it is read and it has no entries.
 *   Too big     A logical buffer of 2^32 bytes or more: GPK_DNSS_ST_TOOBIG,
 *               treated as GPK_DNSS_LOST without reading a byte. The same
 *               holds for a stream whose bytes gpk_tcpasm_batch did not write
 *               (past its data_cap), and for a tail outside in->tails
 *               (GPK_DNSS_ST_BADTAIL).
 *   Work cap    in->max_msg_len; 0 means 65535, which is no cap. gpk_dns.h
 *               documents that a crafted message costs about len^2 / 100
 *               dependent loads in one lane and tells callers to bound caplen.
 *               A stream message is bounded by its 16-bit prefix instead, so
 *               caplen does not help here: max_msg_len is this pass's
 *               equivalent of the snap length. A message longer than it is
 *               framed over and gets an entry with status
 *               GPK_DNSS_MSG_SKIPPED: len is set, err is 0, no entries.
 *               Without it the result is the reference's at the reference's
 *               cost.
 *
 * Capacity rule, two levels
 *   Stream      A stream's message entries and its tail are written whole or not
 *               at all, against msg_cap and tail_cap. A stream that does not
 *               fit carries GPK_DNSS_ST_DROPPED: its state and sizes are set
 *               all the same, its messages are not decoded (nfailed is 0).
 *   Message     A placed message's rr entries and names are written whole or
 *               not at all, against rr_cap and name_cap, as GPK_DNS_ST_DROPPED
 *               in gpk_dns.h: here the entry's status carries
 *               GPK_DNSS_MSG_DROPPED (msg.nrr and msg.name_bytes are set).
 *   counts says what a retry needs. The rr and name needs cover the placed
 *   messages only: they are complete once no stream is dropped.
 *
 * Out of scope: DNS.SerializeTo, DoT / DoH / DoQ, and the mDNS and LLMNR
 * ports unless the caller registers them. No gpk_dns_err value is added;
 * gpk_dns_format_error serves as it is.
 *
 * Cost: one lane per stream chases the length prefixes, twice (count, then
 * place): one dependent two-byte read per message and no decode. The decode
 * runs with one lane per message, so a single stream of very many messages
 * (a zone transfer) is decoded by as many lanes.
 */
#ifndef GPK_DNS_STREAMS_H
#define GPK_DNS_STREAMS_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"
#include "gpk_dns.h"
#include "gpk_tcpasm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gpk_dns_stream.state and in->state[j]; meanings and precedence as GPK_TLSS_* */
#define GPK_DNSS_NEW 0     /* input only: first seen in this call                     */
#define GPK_DNSS_SYNCED 1  /* framed so far; tail_len bytes wait for the next call    */
#define GPK_DNSS_NONE 2    /* not a candidate                                         */
#define GPK_DNSS_NOSTART 3 /* no SYN seen                                             */
#define GPK_DNSS_LOST 4    /* bytes were skipped                                      */
#define GPK_DNSS_CLOSED 5  /* ReassemblyComplete                                      */
#define GPK_DNSS_NSTATE 6

/* gpk_dns_stream.status */
#define GPK_DNSS_ST_DROPPED 1u /* its message entries or its tail did not fit a capacity: none was written */
#define GPK_DNSS_ST_TOOBIG 2u  /* logical buffer >= 2^32 bytes, or bytes tcpasm did not write              */
#define GPK_DNSS_ST_BADTAIL 4u /* in->tail_off/tail_len outside in->tails                                  */

/* gpk_dns_stream_msg.status */
#define GPK_DNSS_MSG_PARTIAL 1u /* unfinished at a loss or a close: not decoded                 */
#define GPK_DNSS_MSG_SKIPPED 2u /* longer than in->max_msg_len: not decoded                     */
#define GPK_DNSS_MSG_DROPPED 4u /* decoded, but its entries or names did not fit rr_cap / name_cap */

/* gpk_dns_stream_in.flags */
#define GPK_DNSS_FRAME_UNSTARTED 1u
#define GPK_DNSS_ALL_FLAGS 1u

#define GPK_DNSS_MAX_TAIL 65536u /* 2 + 65535 - 1 */

/* ---- one stream of the call (64 B), in tcpasm's stream order -------------------
 * The stream's logical buffer is its tail (tail_in bytes of in->tails) followed
 * by data[stream_data0[j] .. stream_data0[j+1]) of the assembler's output, cut
 * at the first chunk with Skip > 0. consumed is how far the buffer was framed:
 * the end of the last whole message; tail_len = buffer length - consumed bytes
 * were left for the next call (SYNCED only). msg0 and tail_off are the sums of
 * nmsg and tail_len of the streams in front of it, whether those fitted or not. */
typedef struct gpk_dns_stream {
  uint8_t state;         /*  0 GPK_DNSS_*                                          */
  uint8_t status;        /*  1 GPK_DNSS_ST_*                                       */
  uint16_t reserved;     /*  2 0                                                   */
  uint32_t tail_in;      /*  4 bytes of the carried tail in front of the new bytes */
  uint32_t consumed;     /*  8                                                     */
  uint32_t tail_len;     /* 12 bytes of its tail in the tail arena                 */
  uint64_t tail_off;     /* 16 where they start there                              */
  uint32_t nmsg;         /* 24 message entries, PARTIAL and SKIPPED ones included  */
  uint32_t nfailed;      /* 28 those with err != 0                                 */
  uint64_t msg0;         /* 32 first entry in msgs                                 */
  uint64_t reserved2[3]; /* 40 0                                                   */
} gpk_dns_stream;

/* ---- one message of a stream (80 B), in stream order and, inside a stream, in
 * message order. msg is a gpk_dns as gpk_dns.h defines it, with hdr_off (and
 * the *_off of its entries) relative to the stream's logical buffer, and rr0 /
 * name0 the sums over the placed messages in front of it. A PARTIAL or SKIPPED
 * entry has kind, hdr_off and len set and every other field of msg 0. */
typedef struct gpk_dns_stream_msg {
  gpk_dns msg;         /*  0                                                              */
  uint32_t stream;     /* 64 the stream's index in this call                              */
  uint8_t status;      /* 68 GPK_DNSS_MSG_*                                               */
  uint8_t reserved[3]; /* 69 0                                                            */
  uint32_t present;    /* 72 bytes that were there, the two length bytes included: 2 + len
                             unless PARTIAL                                               */
  uint32_t reserved2;  /* 76 0                                                            */
} gpk_dns_stream_msg;

/* What the streams carry into this call, and the call's options. in == NULL:
 * every stream is new and no option is set. */
typedef struct gpk_dns_stream_in {
  const uint32_t* state;    /* [n] device: GPK_DNSS_NEW or the state a stream had after the last call */
  const uint64_t* tail_off; /* [n] device: its tail is tails[tail_off .. tail_off + tail_len)         */
  const uint32_t* tail_len; /* [n] device                                                             */
  const uint8_t* tails;     /* [tail_bytes] device; may be null when tail_bytes is 0                  */
  uint64_t n;               /* entries given; streams at and past n are new                           */
  uint64_t tail_bytes;
  uint32_t flags;           /* GPK_DNSS_FRAME_UNSTARTED                                               */
  uint32_t max_msg_len;     /* 0: no cap; else messages longer than this are SKIPPED (<= 65535)       */
} gpk_dns_stream_in;

/* Outputs, caller-allocated; max = the number of streams the call can have (the
 * batch size n always suffices). S = counts[0] stream entries are written,
 * nothing at or past S, and nothing at or past a capacity. */
typedef struct gpk_dns_stream_out {
  gpk_dns_stream* streams;  /* [max] 8-byte aligned                                                  */
  gpk_dns_stream_msg* msgs; /* [msg_cap] 8-byte aligned; may be null when msg_cap is 0               */
  gpk_dns_rr* rrs;          /* [rr_cap] 8-byte aligned; may be null when rr_cap is 0                 */
  uint8_t* names;           /* [name_cap] may be null when name_cap is 0                             */
  uint8_t* tails;           /* [tail_cap] may be null when tail_cap is 0                             */
  uint64_t* counts;         /* [12] streams S, streams framed, message entries, failed messages
                                    (of the placed ones), overflow (1: something was dropped), then
                                    the needs: message entries [5], rr entries [6], name bytes [7],
                                    tail bytes [8]; [9], [10], [11] are 0                             */
  uint64_t msg_cap;
  uint64_t rr_cap;
  uint64_t name_cap;
  uint64_t tail_cap;
} gpk_dns_stream_out;

typedef struct gpk_dns_stream_decoder gpk_dns_stream_decoder;

/* Workspace of the scans for calls of up to max_streams (< 2^28) streams and
 * msg_cap <= max_msgs (< 2^28) message entries on one device: a few dozen bytes
 * per stream and per message and nothing per byte. The message that straddles
 * a carried tail and the new bytes is decoded in place through a two-buffer
 * byte accessor, so no seam copy and no 64 KiB per stream is set aside. It
 * serves one call at a time. */
int gpk_dns_stream_decoder_create(gpk_dns_stream_decoder** out, int device, uint64_t max_streams, uint64_t max_msgs);
int gpk_dns_stream_decoder_destroy(gpk_dns_stream_decoder* d);

/* Decode the DNS messages of the streams of one gpk_tcpasm_batch call. batch
 * and res (records + layouts) are the assembler's inputs, asm_out its outputs,
 * all device-resident; the numbers of streams and of messages stay on the
 * device. Asynchronous on `stream`; no host synchronisation or readback
 * happens inside; the caller's HIP device is restored. GPK_EINVAL: a null
 * argument, batch->n > max_streams, out->msg_cap > max_msgs, unknown flags,
 * max_msg_len > 65535, streams, msgs or rrs not 8-byte aligned, an arena null
 * with a capacity > 0, in->n > batch->n. */
int gpk_dns_streams(gpk_dns_stream_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                    const gpk_results* res, const gpk_tcp_streams* asm_out, const gpk_dns_stream_in* in,
                    const gpk_dns_stream_out* out, void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The rules are the ones the kernels run. */
int gpk_dns_streams_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                         const gpk_tcp_streams* host_asm_out, const gpk_dns_stream_in* in,
                         const gpk_dns_stream_out* host_out);

#ifdef __cplusplus
}
#endif
#endif /* GPK_DNS_STREAMS_H */
