/*
 * gpk_tls_streams.h — decode the TLS records of reassembled TCP streams on the
 * device: gpk_tcpasm_batch (gpk_tcpasm.h) lays every stream's
 * bytes out contiguously, gpk_tls_rules.h decodes a TLS record from a buffer;
 * this entry group is the step between them. It finds the record boundaries
 * of every stream, keeps an unfinished record across calls and runs
 * TLS.DecodeFromBytes (layers/tls.go:118-194) on each whole record.
 *
 * The reference has no such entry. The result is defined as what this Go
 * program on top of tcpassembly produces for one stream instance (one
 * direction), over the bytes its Reassembled calls deliver in order:
 *     read 5 header bytes; read Length more bytes;
 *     rec := make([]byte, 5+Length) holding exactly that record;
 *     (&layers.TLS{}).DecodeFromBytes(rec, gopacket.NilDecodeFeedback)
 * Every record is one DecodeFromBytes call on a buffer of exactly its own
 * bytes (len == cap == 5 + Length), so every entry is something gpk_tls.h
 * already defines (line numbers as there: tls.go, tls_handshake.go = hs).
 *
 * Rules
 *   Record      A whole record gives its gpk_tls_rec fields, a ClientHello its
 *               gpk_tls_hello and its server name. A record that fails on its
 *               own is a failed entry with the reference's error, arguments
 *               and Truncated: a CCS of length != 1 (ccs:43-46), a short alert
 *               (al:80-83), "Unknown TLS handshake type" for a plaintext
 *               ServerHello (hs:245-246), "TLS handshake record too short"
 *               (hs:235-238), the five ClientHello length errors (hs:113-159)
 *               and the 0xFFF8..0xFFFF host-name panic (hs:179-180). Framing
 *               goes on behind a failed record: its length is known. A failed
 *               entry keeps the header's content_type, version and length and
 *               its body_off; hs, v0, v1 are 0 and hello is GPK_TLS_NO_HELLO.
 *   Buffer end  DEPARTURE from the per-packet pass (gpk_tls.h, ClientHello):
 *               hs:110 re-slices the body to data[:cap(data)], and here the
 *               buffer ends with the record, so a ClientHello cannot read into
 *               the next record. A ClientHello that overruns its record fails
 *               with one of the five length errors.
 *   Not TLS     A header (5 bytes) whose content type is outside 20..23 ends
 *               the stream as GPK_TLSS_NOT_TLS (:146-148): one last failed
 *               entry with GPK_TLS_ERR_RECORD_TYPE (the header's fields,
 *               body_off behind the header); nothing behind it is looked at,
 *               in this call or any later one.
 *   Loss        A chunk with Skip > 0 ends the stream as GPK_TLSS_LOST. The
 *               bytes in front of the gap are framed; an unfinished record in
 *               front of the gap becomes one last failed entry with what
 *               DecodeFromBytes(tail) returns: "TLS record too short" under 5
 *               bytes (:131-134; content_type, version and length are 0) or
 *               "TLS packet length mismatch" (:150-155), both Truncated.
 *               Nothing behind the gap is decoded.
 *   Close       stream_closed != GPK_TCPASM_OPEN with an unfinished record
 *               gives the same last truncated entry; the state is
 *               GPK_TLSS_CLOSED (also without one). A loss wins over a close.
 *   No start    A chunk with Skip == -1 (no SYN seen: it can only be a
 *               stream's first) gives GPK_TLSS_NOSTART and no entries. With
 *               GPK_TLSS_FRAME_UNSTARTED such a stream is framed from its
 *               first byte instead.
 *   Synced      Otherwise the stream stays GPK_TLSS_SYNCED and its unfinished
 *               tail (fewer than 5 header bytes, or a header and a part of the
 *               body) is copied to the tail arena, to be handed back in front
 *               of the stream's bytes of the next call. Length is 16 bits: a
 *               tail is at most 5 + 65535 - 1 = GPK_TLSS_MAX_TAIL bytes.
 *   Candidates  A stream is decoded when the TCP header of its creating packet
 *               (stream_first[j]; the layout slot's last TCP, the harness rule
 *               of gpk_tcpasm.h) leads to LayerTypeTLS: TCP.NextLayerType() as
 *               tcp.go:591-597 writes it, destination port first, then source,
 *               looked up in the parser's tables, so
 *               RegisterTCPPortLayerType(8443, LayerTypeTLS) counts. The
 *               payload may be empty (a SYN has none). The server-to-client
 *               direction is a candidate too. Other streams get GPK_TLSS_NONE.
 *   Carried     in->state[j] other than NEW or SYNCED is final: the stream
 *               keeps it, nothing of it is read and it has no entries.
 *   Too big     A logical buffer of 2^32 bytes or more: GPK_TLSS_ST_TOOBIG,
 *               treated as GPK_TLSS_LOST without reading a byte. The same
 *               holds for a stream whose bytes gpk_tcpasm_batch did not write
 *               (past its data_cap), and for a tail outside in->tails
 *               (GPK_TLSS_ST_BADTAIL).
 *
 * Out of scope: a ClientHello handshake message fragmented over several TLS
 * records, ServerHello and certificate decoding, DTLS and QUIC (DNS over TCP
 * streams is gpk_dns_streams.h). No gpk_tls_err value is added.
 *
 * Cost: one lane frames one stream, twice (sizes, then entries): one dependent
 * header read per record, not per byte. A single stream of very many records
 * is walked by one lane (DESIGN.md §25 records the time).
 */
#ifndef GPK_TLS_STREAMS_H
#define GPK_TLS_STREAMS_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"
#include "gpk_tcpasm.h"
#include "gpk_tls.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gpk_tls_stream.state and in->state[j] */
#define GPK_TLSS_NEW 0     /* input only: first seen in this call                     */
#define GPK_TLSS_SYNCED 1  /* framed so far; tail_len bytes wait for the next call    */
#define GPK_TLSS_NONE 2    /* not a candidate                                         */
#define GPK_TLSS_NOSTART 3 /* no SYN seen                                             */
#define GPK_TLSS_NOT_TLS 4 /* a header with a content type outside 20..23             */
#define GPK_TLSS_LOST 5    /* bytes were skipped                                      */
#define GPK_TLSS_CLOSED 6  /* ReassemblyComplete                                      */
#define GPK_TLSS_NSTATE 7

/* gpk_tls_stream.status */
#define GPK_TLSS_ST_DROPPED 1u /* its entries, names or tail did not fit a capacity: none was written */
#define GPK_TLSS_ST_TOOBIG 2u  /* logical buffer >= 2^32 bytes, or bytes tcpasm did not write         */
#define GPK_TLSS_ST_BADTAIL 4u /* in->tail_off/tail_len outside in->tails                             */

/* gpk_tls_stream_in.flags */
#define GPK_TLSS_FRAME_UNSTARTED 1u
#define GPK_TLSS_ALL_FLAGS 1u

#define GPK_TLSS_MAX_TAIL 65539u /* 5 + 65535 - 1 */

/* ---- one stream of the call (64 B), in tcpasm's stream order -------------------
 * The stream's logical buffer is its tail (tail_in bytes of in->tails) followed
 * by data[stream_data0[j] .. stream_data0[j+1]) of the assembler's output, cut
 * at the first chunk with Skip > 0. Every offset of its entries (body_off, the
 * hello's *_off) is relative to that buffer: off - tail_in indexes this call's
 * stream bytes. consumed is how far the buffer was framed: the end of the last
 * whole record, or of the header that ended the stream as NOT_TLS; tail_len =
 * buffer length - consumed bytes were left for the next call (SYNCED only).
 * rec0, hello0, sni0 and tail_off are the sums of nrec, nhello, sni_bytes and
 * tail_len of the streams in front of it, whether those fitted or not. */
typedef struct gpk_tls_stream {
  uint8_t state;      /*  0 GPK_TLSS_*                                          */
  uint8_t status;     /*  1 GPK_TLSS_ST_*                                       */
  uint16_t reserved;  /*  2 0                                                   */
  uint32_t tail_in;   /*  4 bytes of the carried tail in front of the new bytes */
  uint32_t consumed;  /*  8                                                     */
  uint32_t tail_len;  /* 12 bytes of its tail in the tail arena                 */
  uint64_t tail_off;  /* 16 where they start there                              */
  uint32_t nrec;      /* 24 record entries, the failed ones included            */
  uint32_t nfailed;   /* 28 those with err != 0                                 */
  uint32_t nhello;    /* 32 ClientHellos decoded                                */
  uint32_t sni_bytes; /* 36 bytes of all its server names                       */
  uint64_t rec0;      /* 40 first entry in recs                                 */
  uint64_t hello0;    /* 48 first entry in hellos                               */
  uint64_t sni0;      /* 56 first byte in snis                                  */
} gpk_tls_stream;

/* ---- one record of a stream (32 B), in stream order ------------------------------ */
typedef struct gpk_tls_stream_rec {
  gpk_tls_rec rec;   /*  0 as gpk_tls.h; body_off relative to the logical buffer, hello counted from
                           the stream's hello0                                                      */
  uint8_t err;       /* 16 0, gpk_tls_err or GPK_ERR_PANIC_SLICE_B                                  */
  uint8_t status;    /* 17 GPK_TLS_ST_TRUNCATED                                                     */
  uint16_t reserved; /* 18 0                                                                        */
  uint32_t err_a0;   /* 20                                                                          */
  uint32_t err_a1;   /* 24                                                                          */
  uint32_t stream;   /* 28 the stream's index in this call                                          */
} gpk_tls_stream_rec;

/* What the streams carry into this call, and the call's options. in == NULL:
 * every stream is new and no option is set. */
typedef struct gpk_tls_stream_in {
  const uint32_t* state;    /* [n] device: GPK_TLSS_NEW or the state a stream had after the last call */
  const uint64_t* tail_off; /* [n] device: its tail is tails[tail_off .. tail_off + tail_len)         */
  const uint32_t* tail_len; /* [n] device                                                             */
  const uint8_t* tails;     /* [tail_bytes] device; may be null when tail_bytes is 0                  */
  uint64_t n;               /* entries given; streams at and past n are new                           */
  uint64_t tail_bytes;
  uint32_t flags;           /* GPK_TLSS_FRAME_UNSTARTED                                               */
  uint32_t reserved;        /* 0                                                                      */
} gpk_tls_stream_in;

/* Outputs, caller-allocated; max = the number of streams the call can have (the
 * batch size n always suffices). S = counts[0] stream entries are written,
 * nothing at or past S, and nothing at or past a capacity. Capacity rule, as
 * gpk_tls.h: a stream's entries, names and tail are written only when its
 * whole range fits every capacity; otherwise it carries GPK_TLSS_ST_DROPPED
 * (its state and sizes are set all the same) and counts says what a retry
 * needs. hellos[k].packet holds the stream's index. */
typedef struct gpk_tls_stream_out {
  gpk_tls_stream* streams;  /* [max] 8-byte aligned                                                  */
  gpk_tls_stream_rec* recs; /* [rec_cap] 8-byte aligned; may be null when rec_cap is 0               */
  gpk_tls_hello* hellos;    /* [hello_cap] 8-byte aligned; may be null when hello_cap is 0           */
  uint8_t* snis;            /* [sni_cap] may be null when sni_cap is 0                               */
  uint8_t* tails;           /* [tail_cap] may be null when tail_cap is 0                             */
  uint64_t* counts;         /* [12] streams S, streams decoded (a candidate that was framed), record
                                    entries, failed records, hellos, overflow (1: something was
                                    dropped), then the needs: record entries [6], hello entries [7],
                                    server name bytes [8], tail bytes [9]; [10], [11] are 0           */
  uint64_t rec_cap;
  uint64_t hello_cap;
  uint64_t sni_cap;
  uint64_t tail_cap;
} gpk_tls_stream_out;

typedef struct gpk_tls_stream_decoder gpk_tls_stream_decoder;

/* Workspace of the scans for calls of up to max_streams (< 2^28) streams on one
 * device: a few dozen bytes per stream and nothing per byte. The record that
 * straddles a carried tail and the new bytes is decoded in place through a
 * two-buffer byte accessor, so no seam copy and no 64 KiB per stream is set
 * aside. It serves one call at a time. */
int gpk_tls_stream_decoder_create(gpk_tls_stream_decoder** out, int device, uint64_t max_streams);
int gpk_tls_stream_decoder_destroy(gpk_tls_stream_decoder* d);

/* Decode the TLS records of the streams of one gpk_tcpasm_batch call. batch
 * and res (records + layouts) are the assembler's inputs, asm_out its outputs,
 * all device-resident; the number of streams is read from asm_out->counts[0]
 * on the device. Asynchronous on `stream`; no host synchronisation or readback
 * happens inside; the caller's HIP device is restored. GPK_EINVAL: a null
 * argument, batch->n > max_streams, unknown flags, streams, recs or hellos not
 * 8-byte aligned, an arena null with a capacity > 0, in->n > batch->n. */
int gpk_tls_streams(gpk_tls_stream_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                    const gpk_results* res, const gpk_tcp_streams* asm_out, const gpk_tls_stream_in* in,
                    const gpk_tls_stream_out* out, void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The rules are the ones the kernels run. */
int gpk_tls_streams_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                         const gpk_tcp_streams* host_asm_out, const gpk_tls_stream_in* in,
                         const gpk_tls_stream_out* host_out);

#ifdef __cplusplus
}
#endif
#endif /* GPK_TLS_STREAMS_H */
