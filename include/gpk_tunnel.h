/*
 * gpk_tunnel.h — decode through GRE, VXLAN and Geneve headers on the device
 * (DESIGN.md §19).
 *
 * The decode path ends at the first tunnel header: UDP 4789 leads to
 * LayerTypeVXLAN (116), UDP 6081 to LayerTypeGeneve (120), IP protocol 47 to
 * LayerTypeGRE (18) (layers/ports.go:156,164, enums.go), and the parser has no
 * decoder for them. A Go caller adds &layers.GRE{}, &layers.VXLAN{} and
 * &layers.Geneve{} to its DecodingLayerParser (layers_decoder.go:60-79). This
 * entry group is that step for a decoded batch: it decodes the tunnel header of
 * every packet whose decode stopped at one, bit-exactly with the reference's
 * DecodeFromBytes (layers/gre.go:40-128, vxlan.go:53-78, geneve.go:59-119),
 * error texts and run-time panics included, and hands back the inner packets
 * as a zero-copy gpk_batch per inner first layer, ready for gpk_decode_batch.
 *
 * Rules
 *   Candidate   A packet is a candidate when the NextLayerType() of the last
 *               layer of its decoded list is one of the enabled tunnel types
 *               and that layer's LayerPayload() is not empty (an empty payload
 *               ends DecodeLayers with success before the next type is looked
 *               at, layers_decoder.go:71-73). Both values are recomputed from
 *               the last layer's gpk_layout slot with the parser's tables, so
 *               gpk_parser_set_* edits count, as does a parser with
 *               ignore_unsupported. A decoded list longer than 16 entries
 *               gives GPK_TUN_UNKNOWN (the record names only the first 16).
 *   Slice       The tunnel's DecodeFromBytes gets that payload: len = its
 *               length, cap = the bytes to the end of the packet (the rule of
 *               the MPTCP option panics of the TCP decoder).
 *   Levels      Harness rule, fixed here as the L4 pseudo-header rule is
 *               (DESIGN.md §12): checksum and flow outputs are reported per
 *               level. The inner slices of a call are the packets of the next
 *               level; each level's record is an ordinary gpk_record of that
 *               level's slice. The composed decoded list is outer + [tunnel]
 *               + inner, the composed error is the inner's (or the tunnel's),
 *               Truncated is the OR of the three, and every layer struct holds
 *               its innermost instance (one struct per type, parser.go:21-28).
 */
#ifndef GPK_TUNNEL_H
#define GPK_TUNNEL_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_LT_GRE 18
#define GPK_LT_VXLAN 116
#define GPK_LT_GENEVE 120

/* kinds mask of gpk_tunnel_batch and gpk_tunnel.kind */
#define GPK_TUN_GRE 1u
#define GPK_TUN_VXLAN 2u
#define GPK_TUN_GENEVE 4u
#define GPK_TUN_ALL 7u

/* flags */
#define GPK_TUN_GRE_CSUM 1u /* GRE.VerifyChecksum for the GRE headers with the C bit */

/* verdict[i] of a packet that is not in the compact list */
#define GPK_TUN_NONE (-1)    /* not a candidate */
#define GPK_TUN_UNKNOWN (-2) /* decoded list longer than 16 entries */

/* classes of the compact list, in list order */
#define GPK_TUN_CLASS_ETHERNET 0 /* the inner slice starts at the parser's Ethernet decoder */
#define GPK_TUN_CLASS_DOT1Q 1    /* ... Dot1Q   */
#define GPK_TUN_CLASS_IPV4 2     /* ... IPv4    */
#define GPK_TUN_CLASS_IPV6 3     /* ... IPv6    */
#define GPK_TUN_CLASS_NOINNER 4  /* tunnel decoded; the next type has none of those four decoders,
                                    is 0, or the inner payload is empty */
#define GPK_TUN_CLASS_FAILED 5   /* the tunnel's DecodeFromBytes returned an error or panicked */
#define GPK_TUN_NCLASS 6

/* ---- error sites of the three DecodeFromBytes -----------------------------
 * gpk_tunnel.err is 0, one of these, or one of the three panic forms of gpk.h
 * (GPK_ERR_PANIC_INDEX, GPK_ERR_PANIC_SLICE_ACAP, GPK_ERR_PANIC_SLICE_B with
 * their two arguments). gpk_tunnel_format_error renders Go's text. */
enum gpk_tun_err {
  GPK_TUN_ERR_VXLAN_SMALL = 70,     /* vxlan.go:55   "vxlan packet too small"            */
  GPK_TUN_ERR_GRE_SMALL = 71,       /* gre.go:43     "GRE packet too small"   Truncated  */
  GPK_TUN_ERR_GRE_TRUNCATED = 72,   /* gre.go:47     "GRE packet truncated"   Truncated  */
  GPK_TUN_ERR_GENEVE_OPT_SHORT = 73,/* geneve.go:62  "geneve option too small" Truncated */
  GPK_TUN_ERR_GENEVE_OPT_LEN = 74,  /* geneve.go:73  "geneve option too small" Truncated */
  GPK_TUN_ERR_GENEVE_SHORT = 75,    /* geneve.go:84  "geneve packet too short" Truncated */
  GPK_TUN_ERR_GENEVE_OPTS_SHORT = 76/* geneve.go:102 "geneve packet too short" Truncated */
};

/* gpk_tunnel.status */
#define GPK_TUN_ST_TRUNCATED 1u /* the layer called SetTruncated                              */
#define GPK_TUN_ST_CSUM 2u      /* GRE: the sum was computed, gre_correct holds Correct        */
#define GPK_TUN_ST_VALID 4u     /* GRE with GPK_TUN_GRE_CSUM: Valid (gre.go:246; set without
                                   a sum when the C bit is clear)                             */
/* gpk_tunnel.bits */
#define GPK_TUN_VX_I 1u  /* VXLAN.ValidIDFlag  data[0] & 0x08 */
#define GPK_TUN_VX_G 2u  /* VXLAN.GBPExtension data[0] & 0x80 */
#define GPK_TUN_VX_D 4u  /* VXLAN.GBPDontLearn data[1] & 0x40 */
#define GPK_TUN_VX_A 8u  /* VXLAN.GBPApplied   data[1] & 0x80 */
#define GPK_TUN_GN_O 1u  /* Geneve.OAMPacket      data[1] & 0x80 */
#define GPK_TUN_GN_C 2u  /* Geneve.CriticalOption data[1] & 0x40 */

/* ---- one decoded tunnel header (72 B) --------------------------------------
 * Offsets are relative to the start of the packet of the level's batch.
 * A failed decode (err != 0) has kind, err, err_a0, err_a1, status and hdr_off
 * set and every other field 0.
 *
 * GRE: every boolean and small field derives from the two raw flag bytes:
 *   ChecksumPresent raw0&0x80, RoutingPresent raw0&0x40, KeyPresent raw0&0x20,
 *   SeqPresent raw0&0x10, StrictSourceRoute raw0&0x08, RecursionControl raw0&7,
 *   AckPresent raw1&0x80, Flags raw1>>3, Version raw1&7 (gre.go:63-71; the
 *   version is not checked). The checksum/offset word is present when C or R is
 *   set. The GRERouting list: `count` entries starting at packet byte list_off;
 *   entry: AddressFamily be16, SREOffset u8, SRELength u8, RoutingInformation
 *   [SRELength]; the terminating entry (AddressFamily 0, SRELength 0) follows
 *   the last one and is not counted (gre.go:96-118).
 * Geneve: `count` options; the first starts at packet byte list_off (= hdr_off
 *   + 8). Option j is found by the reference's walk: at header byte o (a uint8,
 *   first 8): Class be16 at o, Type at o+2, Flags = hdr[o+3] >> 5, Length =
 *   (hdr[o+3] & 0x1f) * 4 + 4, Data = hdr[o+4 : o+Length]; o = (o + Length) mod
 *   256 (geneve.go:59-79, :105-114: the offset is a uint8 and wraps; Contents
 *   and Payload are cut at the wrapped offset, so contents_len < 8 happens).
 *   raw0/raw1 are the first two header bytes of every kind. */
typedef struct gpk_tunnel {
  uint8_t kind;          /*  0 GPK_TUN_GRE / _VXLAN / _GENEVE                         */
  uint8_t err;           /*  1 0, gpk_tun_err or a GPK_ERR_PANIC_* code               */
  uint8_t status;        /*  2 GPK_TUN_ST_*                                           */
  uint8_t bits;          /*  3 GPK_TUN_VX_* / GPK_TUN_GN_*                            */
  uint32_t err_a0;       /*  4                                                        */
  uint32_t err_a1;       /*  8                                                        */
  uint32_t hdr_off;      /* 12 packet offset of the tunnel header (the slice)         */
  uint32_t contents_len; /* 16 len(LayerContents()); a GRE routing list is unbounded  */
  uint32_t inner_off;    /* 20 packet offset of LayerPayload()                        */
  uint32_t inner_len;    /* 24 len(LayerPayload())                                    */
  int32_t next_type;     /* 28 NextLayerType()                                        */
  uint32_t vni;          /* 32 VXLAN.VNI / Geneve.VNI                                 */
  uint16_t protocol;     /* 36 GRE.Protocol / Geneve.Protocol                         */
  uint16_t gbp_id;       /* 38 VXLAN.GBPGroupPolicyID                                 */
  uint8_t raw0;          /* 40 header byte 0                                          */
  uint8_t raw1;          /* 41 header byte 1                                          */
  uint16_t gre_checksum; /* 42 GRE.Checksum                                           */
  uint16_t gre_offset;   /* 44 GRE.Offset                                             */
  uint16_t gre_correct;  /* 46 GRE.VerifyChecksum Correct when GPK_TUN_ST_CSUM        */
  uint32_t gre_key;      /* 48 GRE.Key                                                */
  uint32_t gre_seq;      /* 52 GRE.Seq                                                */
  uint32_t gre_ack;      /* 56 GRE.Ack                                                */
  uint32_t count;        /* 60 GRE: listed SREs; Geneve: options                      */
  uint32_t list_off;     /* 64 packet offset of the first SRE / option                */
  uint8_t gn_version;    /* 68 Geneve.Version = data[0] >> 7 (one bit, as written)    */
  uint8_t gn_options_length; /* 69 Geneve.OptionsLength = (data[0] & 0x3f) * 4        */
  uint16_t reserved;     /* 70 0                                                      */
} gpk_tunnel;

/* Outputs, caller-allocated, n = batch size; m = counts[0] <= n entries are
 * written, nothing at or past m. The list is ordered by class and, inside a
 * class, by packet index: the order is a pure function of the batch. */
typedef struct gpk_tunnels {
  int32_t* verdict;      /* [n] position in the compact list, or GPK_TUN_NONE / GPK_TUN_UNKNOWN */
  uint32_t* class_start; /* [7] class c is entries [class_start[c], class_start[c+1])           */
  uint32_t* index;       /* [n] packet id of each entry                                         */
  uint64_t* in_offsets;  /* [n] absolute offset of the inner slice in batch->data               */
  uint32_t* in_caplens;  /* [n] its length (0 for a failed decode)                              */
  gpk_tunnel* tunnels;   /* [n] 8-byte aligned                                                  */
  uint32_t* counts;      /* [8] m, the six class counts, GRE sums computed                      */
} gpk_tunnels;
/* {batch->data, in_offsets + class_start[c], in_caplens + class_start[c],
 * class_start[c+1] - class_start[c], batch->data_bytes} is a gpk_batch for
 * gpk_decode_batch with a parser whose first layer is the class's type. */

typedef struct gpk_tunneler gpk_tunneler;

/* Workspace of the scans for batches of up to max_packets (< 2^32) on one
 * device. It serves one call at a time: calls on one stream are ordered,
 * concurrent streams need one tunneler each. */
int gpk_tunneler_create(gpk_tunneler** out, int device, uint64_t max_packets);
int gpk_tunneler_destroy(gpk_tunneler* t);

/* Peel one tunnel level off a decoded batch. res holds the records and layouts
 * of gpk_decode_batch(ctx, parser, batch); every pointer is device memory;
 * asynchronous on `stream`. kinds: GPK_TUN_* mask; flags: GPK_TUN_GRE_CSUM.
 * GPK_EINVAL: a null argument, kinds 0 or outside GPK_TUN_ALL, unknown flags,
 * batch->n > max_packets, tunnels not 8-byte aligned. */
int gpk_tunnel_batch(gpk_tunneler* t, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                     const gpk_results* res, uint32_t kinds, uint32_t flags, const gpk_tunnels* out,
                     void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The header decoders are the ones the kernels run. */
int gpk_tunnel_batch_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                          uint32_t kinds, uint32_t flags, const gpk_tunnels* host_out);

/* The lane group of the GRE sum: headers + payload of at least `bytes` bytes
 * are summed by 64 lanes, shorter ones by 16 (default GPK_TUN_SUM_GROUP_BYTES).
 * Results do not depend on it. */
#define GPK_TUN_SUM_GROUP_BYTES 8192
int gpk_tunneler_set_sum_threshold(gpk_tunneler* t, uint32_t bytes);

/* Go's error text of a gpk_tunnel (err, err_a0, err_a1); as gpk_format_error. */
int gpk_tunnel_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPK_TUNNEL_H */
