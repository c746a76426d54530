/*
 * gpk_ndp.h — decode the NDP and MLD messages behind ICMPv6 on the device
 * (DESIGN.md §27).
 *
 * ICMPv6.NextLayerType() (layers/icmp6.go:230-261) leads to one of ten message
 * layers and the control pass (gpk_control.h) has no decoder for them. A Go
 * caller adds &layers.ICMPv6RouterSolicitation{}, ...RouterAdvertisement{},
 * ...NeighborSolicitation{}, ...NeighborAdvertisement{}, ...ICMPv6Redirect{},
 * the three MLDv1 and the two MLDv2 message layers to its DecodingLayerParser.
 * This entry group is that step for a decoded batch: for every packet whose
 * decode ends in front of one of them it runs the layer's DecodeFromBytes
 * (layers/icmp6msg.go:190-202, 237-255, 306-319, 355-369, 422-436, 514-546,
 * mldv1.go:32-43, 95-106, mldv2.go:61-90, 309-333, 473-509). The result is
 * not a fixed-size record: the message record (gpk_ndp) names a range of
 * 16-byte entries (gpk_ndp_entry), one per ICMPv6Option or per
 * MLDv2MulticastAddressRecord. Address and option bytes stay in the packet:
 * the arena holds descriptors only.
 *
 * Rules
 *   Candidate   Two ways in, both recomputed from the last decoded layer's
 *               gpk_layout slot and the parser's tables (tun::candidate of
 *               gpk_tunnel.h, unchanged), so table edits and
 *               ignore_unsupported count. A decoded list longer than 16
 *               entries gives GPK_NDP_UNKNOWN.
 *               1. Behind an ICMPv6 header: the last layer's NextLayerType()
 *                  is LayerTypeICMPv6 (57), `kinds` carries GPK_NDP_ICMP6 (the
 *                  caller's parser holds layers.ICMPv6), ctl::decode_icmp6
 *                  succeeds, the ICMPv6's payload is not empty and
 *                  ctl::icmp6_next(type, len(payload)) is an enabled kind.
 *                  The message is the ICMPv6 payload. Type 130 is an MLDv2
 *                  query when that payload is longer than 20 bytes and an
 *                  MLDv1 one otherwise (icmp6.go:249-254).
 *               2. In front, through a table edit: the last layer's
 *                  NextLayerType() is itself an enabled kind. The message is
 *                  that layer's payload.
 *   Loop        Every one of the ten ends the reference's loop
 *               (layers_decoder.go:60-79) with nil. Router Solicitation and
 *               the five MLD layers set no BaseLayer; the other four set
 *               BaseLayer{data, nil}, so their payload is empty.
 *               MLDv1MulticastListenerQueryMessage sets Payload = data[20:]
 *               when len(data) > 20 (reachable only through way 2, since way
 *               1 makes such a message an MLDv2 query); its NextLayerType() is
 *               LayerTypeZero, which has no decoder, so the loop returns
 *               (LayerTypeZero, nil) and DecodeLayers turns that into nil
 *               (parser.go:308-317): payload_off / payload_len record the
 *               range. The composed list gains exactly one layer type and the
 *               composed error becomes nil; on a failure nothing is appended
 *               and the error is the message's.
 *   Options     ICMPv6Options.DecodeFromBytes (icmp6msg.go:514-546): while
 *               bytes are left: fewer than 2; length = data[1] * 8 is 0; fewer
 *               than length; else one option with Data = data[2:length].
 *   Records     MLDv2MulticastAddressRecord.decode (mldv2.go:473-509) over
 *               data[begin:]: fewer than 20 bytes (the text says 4); source i
 *               ends past the data (the text names 20 + 16 (i + 1)); fewer
 *               than 20 + 16 N + 4 AuxDataLen bytes (the text names 20 + 16 N,
 *               the length WITHOUT the auxiliary data, and this one site does
 *               not call SetTruncated).
 *   Guarded     No slice expression of these paths is unguarded: every
 *               data[a:b] sits behind the length check in front of it,
 *               data[begin:] of the report loop has begin <= len(data) because
 *               a record's `read` never exceeds what it was handed, and
 *               data[2:length] has 8 <= length <= len(data). There is no
 *               run-time panic to report.
 *
 * Scope decisions
 *   Fresh struct  Every message is decoded into a fresh struct. The
 *               reference's MLDv2 layers append to SourceAddresses and
 *               MulticastAddressRecords without truncating them, so a struct
 *               reused by a DecodingLayerParser accumulates the lists of
 *               earlier packets (the NDP layers do truncate, Options[:0]), and
 *               the layers that set no BaseLayer keep an earlier packet's.
 *               Here a message's lists and ranges are its own.
 *   Failed      A failed message has no entries: the options or records the
 *               reference had appended in front of the error are not
 *               reported.
 */
#ifndef GPK_NDP_H
#define GPK_NDP_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"
#include "gpk_control.h" /* the ten GPK_LT_* layer types */

#ifdef __cplusplus
extern "C" {
#endif

/* kinds mask of gpk_ndp_batch: the layers the caller's parser holds */
#define GPK_NDP_RS 1u           /* ICMPv6RouterSolicitation            */
#define GPK_NDP_RA 2u           /* ICMPv6RouterAdvertisement           */
#define GPK_NDP_NS 4u           /* ICMPv6NeighborSolicitation          */
#define GPK_NDP_NA 8u           /* ICMPv6NeighborAdvertisement         */
#define GPK_NDP_REDIRECT 16u    /* ICMPv6Redirect                      */
#define GPK_NDP_MLD1_QUERY 32u  /* MLDv1MulticastListenerQueryMessage  */
#define GPK_NDP_MLD1_REPORT 64u /* MLDv1MulticastListenerReportMessage */
#define GPK_NDP_MLD1_DONE 128u  /* MLDv1MulticastListenerDoneMessage   */
#define GPK_NDP_MLD2_QUERY 256u /* MLDv2MulticastListenerQueryMessage  */
#define GPK_NDP_MLD2_REPORT 512u /* MLDv2MulticastListenerReportMessage */
#define GPK_NDP_MESSAGES 1023u
#define GPK_NDP_ICMP6 1024u     /* layers.ICMPv6: opens way 1; alone it is GPK_EINVAL */
#define GPK_NDP_ALL 2047u

/* verdict[i] of a packet that is not in the compact list */
#define GPK_NDP_NONE (-1)    /* not a candidate */
#define GPK_NDP_UNKNOWN (-2) /* decoded list longer than 16 entries */

/* classes of the compact list, in list order */
#define GPK_NDP_CLASS_OK 0
#define GPK_NDP_CLASS_FAILED 1 /* DecodeFromBytes returned an error */
#define GPK_NDP_NCLASS 2

/* gpk_ndp.err; gpk_ndp_format_error renders Go's text. Every site but the last calls SetTruncated. */
enum gpk_ndp_err {
  GPK_NDP_ERR_RS_SHORT = 140,  /* icmp6msg.go:193 "ICMP layer less then 4 bytes for ICMPv6 router solicitation"      */
  GPK_NDP_ERR_RA_SHORT,        /* :238 "ICMP layer less then 12 bytes for ICMPv6 router advertisement"              */
  GPK_NDP_ERR_NS_SHORT,        /* :307 "ICMP layer less then 20 bytes for ICMPv6 neighbor solicitation"             */
  GPK_NDP_ERR_NA_SHORT,        /* :356 "ICMP layer less then 20 bytes for ICMPv6 neighbor advertisement"            */
  GPK_NDP_ERR_REDIRECT_SHORT,  /* :423 "ICMP layer less then 36 bytes for ICMPv6 redirect"                          */
  GPK_NDP_ERR_OPT_SHORT,       /* :516 "ICMP layer less then 2 bytes for ICMPv6 message option"                     */
  GPK_NDP_ERR_OPT_ZERO,        /* :524 "ICMPv6 message option with length 0"                                        */
  GPK_NDP_ERR_OPT_OVERRUN,     /* :529 "ICMP layer only %v bytes for ICMPv6 message option with length %v"
                                       (a0 bytes left, a1 length)                                                    */
  GPK_NDP_ERR_MLD1_SHORT,      /* mldv1.go:33 "ICMP layer less than 20 bytes for Multicast Listener Query Message V1"
                                       (Report and Done use the same text)                                           */
  GPK_NDP_ERR_MLD2_QUERY_SHORT,/* mldv2.go:62 "ICMP layer less than 24 bytes for Multicast Listener Query Message V2" */
  GPK_NDP_ERR_MLD2_QUERY_SOURCES, /* :81 "ICMP layer less than %d bytes for Multicast Listener Query Message V2" (a0 end) */
  GPK_NDP_ERR_MLD2_REPORT_SHORT,  /* :310 "ICMP layer less than 4 bytes for Multicast Listener Report Message V2"    */
  GPK_NDP_ERR_RECORD_SHORT,    /* :474 "Multicast Listener Report Message V2 layer less than 4 bytes for Multicast
                                       Address Record" (the check is < 20)                                           */
  GPK_NDP_ERR_RECORD_SOURCES,  /* :489 "Multicast Listener Report Message V2 layer less than %d bytes for Multicast
                                       Address Record" (a0 end)                                                      */
  GPK_NDP_ERR_RECORD_AUX,      /* :500 the same text (a0 = 20 + 16 N, without the auxiliary data); NOT Truncated     */
  GPK_NDP_ERR_END
};

/* gpk_ndp.status */
#define GPK_NDP_ST_TRUNCATED 1u /* DecodeFromBytes called SetTruncated                                    */
#define GPK_NDP_ST_DROPPED 2u   /* the message decoded, but its entries did not fit entry_cap: none written */

/* ---- one candidate (64 B) ----------------------------------------------------
 * Offsets are relative to the start of the packet; the message is
 * packet[hdr_off : hdr_off + len]. contents_len is len(LayerContents()): len
 * for the four layers that set BaseLayer{data, nil}, 0 for the others.
 * payload_off / payload_len are LayerPayload(): the bytes behind the 20 of an
 * MLDv1 query, 0 / 0 everywhere else. The message's entries are
 * entries[entry0 .. entry0 + nentries): its options, or the records of an
 * MLDv2 report; entry0 is the sum of nentries of the entries in front of it
 * in the compact list, whether those fitted or not. v[] by layer type (0
 * where unused):
 *   RouterAdvertisement    v0 ReachableTime, v1 RetransTimer, v2 RouterLifetime,
 *                          v3 HopLimit; flags is Flags
 *   NeighborSolicitation   v0 packet offset of TargetAddress (16 bytes)
 *   NeighborAdvertisement  the same; flags is Flags
 *   Redirect               v0 packet offset of TargetAddress, v1 of
 *                          DestinationAddress
 *   MLDv1 Query/Report/Done v0 packet offset of MulticastAddress, v2 the raw 16
 *                          bits of MaximumResponseDelay (milliseconds)
 *   MLDv2 Query            v0 packet offset of MulticastAddress, v2
 *                          MaximumResponseCode; s_qrv is data[20] & 0xF
 *                          (SuppressRoutersideProcessing = s_qrv & 8,
 *                          QueriersRobustnessVariable = s_qrv & 7), qqic
 *                          QueriersQueryIntervalCode, count NumberOfSources;
 *                          SourceAddresses are the 16 count bytes at
 *                          hdr_off + 24: contiguous, they need no entry
 *   MLDv2 Report           count NumberOfMulticastAddressRecords (= nentries)
 * A failed message (class FAILED) has layer_type, err, err_a0, err_a1, status
 * and hdr_off set and every other field 0: no entries. */
typedef struct gpk_ndp {
  uint8_t layer_type;    /*  0 GPK_LT_* of the message layer (124..128, 135..139) */
  uint8_t err;           /*  1 0 or gpk_ndp_err                                   */
  uint8_t status;        /*  2 GPK_NDP_ST_*                                       */
  uint8_t flags;         /*  3 RouterAdvertisement.Flags / NeighborAdvertisement.Flags */
  uint32_t err_a0;       /*  4                                                    */
  uint32_t err_a1;       /*  8                                                    */
  uint32_t hdr_off;      /* 12 packet offset of the message                       */
  uint32_t len;          /* 16 its length                                         */
  uint32_t contents_len; /* 20 len(LayerContents())                               */
  uint32_t payload_off;  /* 24 packet offset of LayerPayload()                    */
  uint32_t payload_len;  /* 28 len(LayerPayload())                                */
  uint32_t v[4];         /* 32 the layer's scalars and address offsets            */
  uint64_t entry0;       /* 48 first entry in entries                             */
  uint32_t nentries;     /* 56 options, or multicast address records              */
  uint16_t count;        /* 60 NumberOfSources / NumberOfMulticastAddressRecords  */
  uint8_t s_qrv;         /* 62 MLDv2 query: data[20] & 0xF                        */
  uint8_t qqic;          /* 63 MLDv2 query: QueriersQueryIntervalCode             */
} gpk_ndp;

/* ---- one option or one multicast address record (16 B) -------------------------
 * ICMPv6Option: type is Type, off the packet offset of Data and ext
 * len(Data) (8 data[1] - 2); aux_data_len, n and aux_off are 0.
 * MLDv2MulticastAddressRecord: type is RecordType, aux_data_len AuxDataLen (in
 * 32-bit words), n N; off is the packet offset of MulticastAddress, ext that
 * of the n SourceAddresses (16 n bytes) and aux_off that of AuxiliaryData
 * (4 aux_data_len bytes). */
typedef struct gpk_ndp_entry {
  uint8_t type;         /*  0 */
  uint8_t aux_data_len; /*  1 */
  uint16_t n;           /*  2 */
  uint32_t off;         /*  4 */
  uint32_t ext;         /*  8 */
  uint32_t aux_off;     /* 12 */
} gpk_ndp_entry;

/* Outputs, caller-allocated, n = batch size; m = counts[0] <= n entries of
 * index and records are written, nothing at or past m. The list is ordered by
 * class and, inside a class, by packet index. entries holds entry_cap
 * entries; nothing is written at or past it. A message's entries are written
 * only when its whole range fits (entry0 + nentries <= entry_cap); otherwise
 * its record carries GPK_NDP_ST_DROPPED. counts tells what a retry needs. */
typedef struct gpk_ndps {
  int32_t* verdict;       /* [n] position in the compact list, or GPK_NDP_NONE / GPK_NDP_UNKNOWN */
  uint32_t* class_start;  /* [3] class c is entries [class_start[c], class_start[c+1])           */
  uint32_t* index;        /* [n] packet id of each entry                                         */
  gpk_ndp* records;       /* [n] 8-byte aligned                                                  */
  uint32_t* counts;       /* [8] m, OK, FAILED, overflow (1: something was dropped), entries
                                 needed (low, high dword), 0, 0                                   */
  gpk_ndp_entry* entries; /* [entry_cap] 8-byte aligned; may be null when entry_cap is 0         */
  uint64_t entry_cap;
} gpk_ndps;

typedef struct gpk_ndp_decoder gpk_ndp_decoder;

/* Workspace of the scans for batches of up to max_packets (< 2^28) on one
 * device. It serves one call at a time: calls on one stream are ordered,
 * concurrent streams need one decoder each. */
int gpk_ndp_decoder_create(gpk_ndp_decoder** out, int device, uint64_t max_packets);
int gpk_ndp_decoder_destroy(gpk_ndp_decoder* d);

/* Work per message is linear in its length. One lane walks a message, three
 * times: in the classify and the scatter step (counting) and in the emit
 * step. An option takes at least 8 bytes, a record at least 20 and a source
 * 16 (sources are checked with one division, not walked), and a count that
 * overstates the data fails at the first item that does not fit: a message of
 * len bytes costs at most len / 8 steps. There is no cliff to warn about.
 *
 * Decode the NDP and MLD messages at the end of a decoded batch. res holds the
 * records and layouts of gpk_decode_batch(ctx, parser, batch); every pointer is
 * device memory; batch->data is 16-byte aligned; asynchronous on `stream`; the
 * caller's HIP device is restored. kinds: GPK_NDP_* mask of the layers the
 * caller's parser holds. GPK_EINVAL: a null argument, kinds 0, outside
 * GPK_NDP_ALL or GPK_NDP_ICMP6 alone, batch->n > max_packets, data not
 * 16-byte aligned, records or entries not 8-byte aligned, entries null with
 * entry_cap > 0. */
int gpk_ndp_batch(gpk_ndp_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                  const gpk_results* res, uint32_t kinds, const gpk_ndps* out, void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The walk is the one the kernels run. */
int gpk_ndp_batch_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                       uint32_t kinds, const gpk_ndps* host_out);

/* Go's error text of a gpk_ndp (err, err_a0, err_a1); as gpk_format_error. */
int gpk_ndp_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPK_NDP_H */
