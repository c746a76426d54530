/*
 * gpk_tls.h — decode the TLS records and the ClientHello SNI of a decoded
 * batch on the device.
 *
 * TCP ports 443, 636, 989, 990, 992-995, 5061, 5082 and 5083 lead to
 * LayerTypeTLS (140) in the port tables (layers/ports.go) and the parser has no
 * decoder for it. A Go caller adds &layers.TLS{} to its DecodingLayerParser.
 * This entry group is that step for a decoded batch: for every packet whose
 * decoded list ends in front of LayerTypeTLS it runs TLS.DecodeFromBytes
 * (layers/tls.go:118-194). The result is not a fixed-size record: the message
 * record (gpk_tls) names a range of record entries (gpk_tls_rec, one per TLS
 * record), a range of hello entries (gpk_tls_hello, one per decoded
 * ClientHello) and a range of a byte arena that holds the server names.
 *
 * Rules (line numbers: tls.go, tls_handshake.go = hs, tls_alert.go = al,
 * tls_cipherspec.go = ccs, tls_appdata.go = app)
 *   Candidate   tun::candidate, unchanged (gpk_tunnel.h): the NextLayerType()
 *               of the last layer of the decoded list, recomputed from its
 *               gpk_layout slot with the parser's tables, is 140 and that
 *               layer's LayerPayload() is not empty. Table edits count:
 *               RegisterTCPPortLayerType(8443, LayerTypeTLS) makes 8443 a TLS
 *               port. A decoded list longer than 16 entries gives
 *               GPK_TLS_UNKNOWN.
 *   Loop        TLS.Payload() is nil and NextLayerType() is Zero (:202-209):
 *               the reference's loop ends after it with nil. 140 is appended
 *               to the decoded list, nothing follows.
 *   Records     decodeTLSRecords (:130-194) calls itself on data[tl:] as its
 *               last statement: a loop. Per record, in this order: fewer than
 *               5 bytes left, "TLS record too short", Truncated (:131-134); a
 *               content type outside 20..23, "Unknown TLS record type"
 *               (:146-148; the switch's default at :158 cannot be reached
 *               behind it); fewer than 5 + Length bytes left, "TLS packet
 *               length mismatch", Truncated (:150-155); the per-type decode
 *               of data[5 : 5+Length]; the end when the record ends the data
 *               (:190-192). The work is linear in the message length. The
 *               worst case is a 64 KiB message of `17 03 03 00 00`: about
 *               13 000 valid empty records, each a handful of dependent byte
 *               loads in one lane and, when they fit, a 16-byte entry.
 *   CCS         a body length other than 1: error, Truncated (ccs:43-46);
 *               Message is 1, or 255 for any other byte (ccs:48-51).
 *   Alert       a body shorter than 2: error, Truncated (al:80-83). Length 2:
 *               Level and Description are the body's bytes; otherwise both
 *               are 255 and EncryptedMsg is the body (al:85-92).
 *   AppData     Payload is the body (app:32). app:28 compares len(data) with
 *               Length, and data is data[5 : 5+Length] of a slice the caller
 *               has shown to be that long: its error cannot occur and has no
 *               code.
 *   Handshake   isEncryptedHandshakeMessage first (hs:198-223): Length < 16 is
 *               plaintext; otherwise the record is encrypted when
 *               uint32(Length) - be24(body[1:4]) != 4 in uint32 arithmetic, or
 *               when body[0] is not one of the eleven types of
 *               handShakeTypeMap (0, 1, 2, 3, 11..16, 20). An encrypted record
 *               is kept with its header only, error nil (hs:232-234). A
 *               plaintext one: an empty body, "TLS handshake record too
 *               short", Truncated (hs:235-238); type 1 is a ClientHello; type
 *               16 nothing more; any other type "Unknown TLS handshake type"
 *               (hs:245-246): a plaintext ServerHello, Certificate or
 *               ServerHelloDone fails the whole packet.
 *   ClientHello hs:110 re-slices the body to data[:cap(data)]: it reads past
 *               the record's end, to the end of the buffer. Scope decision: a
 *               packet is a buffer of exactly its captured bytes, as
 *               pcapgo.ReadPacketData makes it (make([]byte, CaptureLength)),
 *               so the capacity ends at offsets[i] + caplens[i] of the batch
 *               entry. On an inner tunnel level that is the inner slice's
 *               end: this departs from Go only when bytes follow the tunnel
 *               payload in the outer packet and a ClientHello overruns its
 *               record. Then the five length checks in int, each with its
 *               own text and Truncated: 39 bytes (hs:113), session ID (:130),
 *               cipher suites (:138), compression methods (:147), extensions
 *               (:157).
 *   Extensions  hs:163-186 over data[pos : pos+ExtensionsLength]: the walk
 *               stops silently on fewer than 4 bytes left or on an extension
 *               longer than the rest. Only type 0 is read, and its reads use
 *               the rest of the extensions block, not the extension's own
 *               bytes: len > 6, list length > 0, entry type 0, len > 8, then
 *               len > int(8 + hostnameLength) with the sum in uint16. The last
 *               server name that passes wins.
 *   Panic       8 + hostnameLength and 9 + hostnameLength are uint16 sums
 *               (hs:179-180). For hostnameLength 0xFFF8..0xFFFF the guard
 *               wraps to 0..7 and passes (len > 8 holds), and
 *               data[9 : 9+hostnameLength] has a high bound h of 1..8 below
 *               its low bound: Go panics with "slice bounds out of range
 *               [9:h]" (the capacity check passes, h <= 8 < len), which
 *               DecodeLayers turns into an error. Reported as
 *               GPK_ERR_PANIC_SLICE_B, a0 = 9, a1 = h. 0xFFF7 gives a guard of
 *               0xFFFF, which no block of at most 65535 bytes exceeds.
 *               data[4+length:] (hs:185) is a uint16 sum too, but hs:169 has
 *               broken the walk for every length with 4 + int(length) >
 *               len(data), and len(data) <= 65535: the sum never wraps. No
 *               other slice expression or conversion of the path is unguarded.
 *   Failure     A failed message has class FAILED, its error, the two
 *               arguments, Truncated and hdr_off; it has no entries: the
 *               records Go had appended in front of the error are not
 *               reported.
 *   Streams     Each packet is decoded on its own, as the reference does: a
 *               ClientHello split over two TCP segments fails with "TLS
 *               packet length mismatch". TLS over reassembled streams is
 *               gpk_tls_streams (gpk_tls_streams.h). ServerHello and
 *               certificate decoding (the reference has none), DTLS, QUIC
 *               and TLS.SerializeTo are not built.
 */
#ifndef GPK_TLS_H
#define GPK_TLS_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_LT_TLS 140

/* kinds mask of the pass */
#define GPK_TLS_KIND 1u
#define GPK_TLS_ALL 1u

/* verdict[i] of a packet that is not in the compact list */
#define GPK_TLS_NONE (-1)    /* not a candidate */
#define GPK_TLS_UNKNOWN (-2) /* decoded list longer than 16 entries */

/* classes of the compact list, in list order */
#define GPK_TLS_CLASS_OK 0
#define GPK_TLS_CLASS_FAILED 1 /* DecodeFromBytes returned an error or panicked */
#define GPK_TLS_NCLASS 2

/* gpk_tls.err: one of these or GPK_ERR_PANIC_SLICE_B (gpk.h); gpk_tls_format_error renders Go's text */
enum gpk_tls_err {
  GPK_TLS_ERR_RECORD_SHORT = 121, /* :133    "TLS record too short"                             Truncated */
  GPK_TLS_ERR_RECORD_TYPE,        /* :147    "Unknown TLS record type"                                    */
  GPK_TLS_ERR_LENGTH_MISMATCH,    /* :154    "TLS packet length mismatch"                       Truncated */
  GPK_TLS_ERR_CCS_LENGTH,         /* ccs:45  "TLS Change Cipher Spec record incorrect length"   Truncated */
  GPK_TLS_ERR_ALERT_SHORT,        /* al:82   "TLS Alert packet too short"                       Truncated */
  GPK_TLS_ERR_HANDSHAKE_SHORT,    /* hs:237  "TLS handshake record too short"                   Truncated */
  GPK_TLS_ERR_HANDSHAKE_TYPE,     /* hs:246  "Unknown TLS handshake type"                                 */
  GPK_TLS_ERR_HELLO_SHORT,        /* hs:115  "TLS ClientHello too short"                        Truncated */
  GPK_TLS_ERR_HELLO_SESSION,      /* hs:132  "TLS ClientHello truncated in session ID"          Truncated */
  GPK_TLS_ERR_HELLO_CIPHERS,      /* hs:140  "TLS ClientHello truncated in cipher suites"       Truncated */
  GPK_TLS_ERR_HELLO_COMPRESSION,  /* hs:149  "TLS ClientHello truncated in compression methods" Truncated */
  GPK_TLS_ERR_HELLO_EXTENSIONS,   /* hs:159  "TLS ClientHello truncated in extensions"          Truncated */
  GPK_TLS_ERR_END
};

/* gpk_tls.status */
#define GPK_TLS_ST_TRUNCATED 1u /* DecodeFromBytes called SetTruncated */
#define GPK_TLS_ST_DROPPED 2u   /* the message decoded, but its entries or server names did not fit
                                   rec_cap / hello_cap / sni_cap: none of them was written            */

/* ---- one candidate (80 B) ----------------------------------------------------
 * hdr_off is relative to the start of the packet; the message is
 * packet[hdr_off : hdr_off + len]. (The reference resets BaseLayer.Contents
 * for every record, tls.go:139: after a decode it is the last record's slice,
 * packet[last body_off - 5 : hdr_off + len].) The message's record entries are
 * recs[rec0 .. rec0 + nrec), its hello entries hellos[hello0 .. hello0 +
 * nhello), its server names snis[sni0 .. sni0 + sni_bytes). rec0, hello0 and
 * sni0 are the sums of nrec, nhello and sni_bytes of the OK entries in front
 * of it, whether those fitted or not. A failed message (class FAILED) has err,
 * err_a0, err_a1, status and hdr_off set and every other field 0. */
typedef struct gpk_tls {
  uint8_t err;         /*  0 0, gpk_tls_err or GPK_ERR_PANIC_SLICE_B         */
  uint8_t status;      /*  1 GPK_TLS_ST_*                                    */
  uint16_t reserved;   /*  2 0                                               */
  uint32_t err_a0;     /*  4                                                 */
  uint32_t err_a1;     /*  8                                                 */
  uint32_t hdr_off;    /* 12 packet offset of the message                    */
  uint32_t len;        /* 16 its length                                      */
  uint32_t nrec;       /* 20 records: nccs + nalert + nhandshake + nappdata  */
  uint32_t nccs;       /* 24 len(TLS.ChangeCipherSpec)                       */
  uint32_t nalert;     /* 28 len(TLS.Alert)                                  */
  uint32_t nhandshake; /* 32 len(TLS.Handshake)                              */
  uint32_t nappdata;   /* 36 len(TLS.AppData)                                */
  uint32_t nhello;     /* 40 ClientHellos decoded                            */
  uint32_t reserved2;  /* 44 0                                               */
  uint64_t sni_bytes;  /* 48 bytes of all its server names                   */
  uint64_t rec0;       /* 56 first entry in recs                             */
  uint64_t hello0;     /* 64 first entry in hellos                           */
  uint64_t sni0;       /* 72 first byte in snis                              */
} gpk_tls;

/* gpk_tls_rec.hs of a handshake record */
#define GPK_TLS_HS_NONE 0         /* not a handshake record                       */
#define GPK_TLS_HS_ENCRYPTED 1    /* isEncryptedHandshakeMessage: the header only */
#define GPK_TLS_HS_CLIENT_HELLO 2 /* hello names its gpk_tls_hello                */
#define GPK_TLS_HS_CLIENT_KEY 3   /* ClientKeyExchange: nothing decoded           */
#define GPK_TLS_NO_HELLO 0xFFFFFFFFu

/* ---- one TLS record (16 B), in message order -------------------------------------
 * The four slices of the Go struct are the entries filtered by content_type,
 * in order. The body (AppData.Payload, Alert.EncryptedMsg) is
 * packet[body_off : body_off + length]. */
typedef struct gpk_tls_rec {
  uint8_t content_type; /*  0 TLSRecordHeader.ContentType, 20..23                      */
  uint8_t hs;           /*  1 GPK_TLS_HS_*                                             */
  uint8_t v0;           /*  2 Alert.Level, or ChangeCipherSpec.Message (1 or 255)      */
  uint8_t v1;           /*  3 Alert.Description                                        */
  uint16_t version;     /*  4 TLSRecordHeader.Version                                  */
  uint16_t length;      /*  6 TLSRecordHeader.Length                                   */
  uint32_t body_off;    /*  8 packet offset of the body                                */
  uint32_t hello;       /* 12 its hello entry, counted from the message's hello0, or
                              GPK_TLS_NO_HELLO                                         */
} gpk_tls_rec;

/* ---- one decoded ClientHello (64 B) ----------------------------------------------
 * Every slice is a slice of the packet: Random is packet[random_off :
 * random_off + 32], SessionID packet[session_id_off : + session_id_length],
 * CipherSuits, CompressionMethods and Extensions likewise with their length
 * fields, SNI packet[sni_off : sni_off + sni_len] when has_sni (a nil SNI
 * otherwise). The same server name bytes are snis[sni_pos .. sni_pos +
 * sni_len). */
typedef struct gpk_tls_hello {
  uint8_t handshake_type;             /*  0 1                                    */
  uint8_t session_id_length;          /*  1                                      */
  uint8_t compression_methods_length; /*  2                                      */
  uint8_t has_sni;                    /*  3 1: SNI is not nil                    */
  uint32_t length;                    /*  4 the 24-bit Length                    */
  uint16_t protocol_version;          /*  8                                      */
  uint16_t cipher_suits_length;       /* 10                                      */
  uint16_t extensions_length;         /* 12                                      */
  uint16_t reserved;                  /* 14 0                                    */
  uint32_t packet;                    /* 16 packet index in the batch            */
  uint32_t random_off;                /* 20                                      */
  uint32_t session_id_off;            /* 24                                      */
  uint32_t cipher_suits_off;          /* 28                                      */
  uint32_t compression_methods_off;   /* 32                                      */
  uint32_t extensions_off;            /* 36                                      */
  uint32_t sni_off;                   /* 40                                      */
  uint32_t sni_len;                   /* 44                                      */
  uint64_t sni_pos;                   /* 48 its server name in snis              */
  uint64_t reserved2;                 /* 56 0                                    */
} gpk_tls_hello;

/* Outputs, caller-allocated, n = batch size; m = counts[0] <= n entries of
 * index and records are written, nothing at or past m. The list is ordered by
 * class and, inside a class, by packet index. recs holds rec_cap entries,
 * hellos hello_cap entries and snis sni_cap bytes; nothing is written at or
 * past a capacity. Capacity rule: a message's entries and names are written
 * only when its whole range fits every capacity (rec0 + nrec <= rec_cap,
 * hello0 + nhello <= hello_cap and sni0 + sni_bytes <= sni_cap); otherwise its
 * record carries GPK_TLS_ST_DROPPED. counts tells what a retry needs. */
typedef struct gpk_tlss {
  int32_t* verdict;      /* [n] position in the compact list, or GPK_TLS_NONE / GPK_TLS_UNKNOWN */
  uint32_t* class_start; /* [3] class c is entries [class_start[c], class_start[c+1])           */
  uint32_t* index;       /* [n] packet id of each entry                                         */
  gpk_tls* records;      /* [n] 8-byte aligned                                                  */
  uint32_t* counts;      /* [12] m, OK, FAILED, overflow (1: something was dropped), then the
                                 needs as (low, high) dwords: record entries [4,5], hello
                                 entries [6,7], server name bytes [8,9]; [10,11] are 0           */
  gpk_tls_rec* recs;     /* [rec_cap] 8-byte aligned; may be null when rec_cap is 0             */
  gpk_tls_hello* hellos; /* [hello_cap] 8-byte aligned; may be null when hello_cap is 0         */
  uint8_t* snis;         /* [sni_cap] may be null when sni_cap is 0                             */
  uint64_t rec_cap;
  uint64_t hello_cap;
  uint64_t sni_cap;
} gpk_tlss;

typedef struct gpk_tls_decoder gpk_tls_decoder;

/* Workspace of the scans for batches of up to max_packets (< 2^28) on one
 * device. It serves one call at a time: calls on one stream are ordered,
 * concurrent streams need one decoder each. */
int gpk_tls_decoder_create(gpk_tls_decoder** out, int device, uint64_t max_packets);
int gpk_tls_decoder_destroy(gpk_tls_decoder* d);

/* Decode the TLS messages at the end of a decoded batch. One lane walks a
 * message, three times: in the classify and the scatter step (sizes only) and
 * in the emit step; the work is linear in the message length (Records, above).
 * res holds the records and layouts of gpk_decode_batch(ctx, parser, batch);
 * every pointer is device memory; batch->data is 16-byte aligned; asynchronous
 * on `stream`; the caller's HIP device is restored. GPK_EINVAL: a null
 * argument, batch->n > max_packets, data not 16-byte aligned, records, recs or
 * hellos not 8-byte aligned, an arena null with a capacity > 0. */
int gpk_tls_batch(gpk_tls_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                  const gpk_results* res, const gpk_tlss* out, void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The walk is the one the kernels run. */
int gpk_tls_batch_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                       const gpk_tlss* host_out);

/* Go's error text of a gpk_tls (err, err_a0, err_a1); as gpk_format_error. */
int gpk_tls_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPK_TLS_H */
