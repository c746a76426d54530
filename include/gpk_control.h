/*
 * gpk_control.h — decode ICMPv4, ICMPv6 (+ICMPv6Echo) and ARP on the device
 * (DESIGN.md §21).
 *
 * The decode path ends in front of these layers: IP protocol 1 leads to
 * LayerTypeICMPv4 (19), IP protocol 58 to LayerTypeICMPv6 (57), EtherType
 * 0x0806 to LayerTypeARP (10), and the parser has no decoder for them. A Go
 * caller adds &layers.ICMPv4{}, &layers.ICMPv6{}, &layers.ICMPv6Echo{} and
 * &layers.ARP{} to its DecodingLayerParser (layers_decoder.go:60-79). This
 * entry group is that step for a decoded batch: for every packet whose decode
 * stopped in front of one of them it runs the layer's DecodeFromBytes
 * (layers/icmp4.go:221-232, icmp6.go:189-198, icmp6msg.go:155-164,
 * arp.go:42-67), goes on with the reference's loop to the end of the packet
 * (one or two layers are appended), and computes VerifyChecksum of the
 * ICMPv4 / ICMPv6 message.
 *
 * Rules
 *   Candidate   As in gpk_tunnel.h: the NextLayerType() of the last layer of
 *               the decoded list is one of the enabled types and that layer's
 *               LayerPayload() is not empty; both come from the last layer's
 *               gpk_layout slot and the parser's tables. A decoded list longer
 *               than 16 entries gives GPK_CTL_UNKNOWN.
 *   Loop        After the first control layer the loop goes on
 *               (layers_decoder.go:60-79): an empty payload ends it with nil;
 *               LayerTypePayload is decoded when the parser holds
 *               gopacket.Payload; LayerTypeICMPv6Echo when `kinds` holds it;
 *               every other type (and those two without their decoder) is
 *               returned: gpk_control.unsupported. ICMPv6Echo never sets its
 *               BaseLayer, so its payload is empty and the loop ends after it.
 *   Checksum    ICMPv4: Fold(ComputeChecksum(Contents‖Payload, 0) − Checksum)
 *               mod 2^32 (icmp4.go:265-276). ICMPv6: the same with the start
 *               value of computeChecksum (tcpip.go:54-69) for the last network
 *               layer of the decoded list (the pseudo-header rule of DESIGN.md
 *               §1, P2/P12): the address words, 58, length & 0xffff, length >>
 *               16. Without a network layer no sum is made (GPK_CTL_ST_NONET).
 */
#ifndef GPK_CONTROL_H
#define GPK_CONTROL_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_LT_ARP 10
#define GPK_LT_ICMPV4 19
#define GPK_LT_ICMPV6 57
#define GPK_LT_ICMPV6_ROUTER_SOLICITATION 124
#define GPK_LT_ICMPV6_ROUTER_ADVERTISEMENT 125
#define GPK_LT_ICMPV6_NEIGHBOR_SOLICITATION 126
#define GPK_LT_ICMPV6_NEIGHBOR_ADVERTISEMENT 127
#define GPK_LT_ICMPV6_REDIRECT 128
#define GPK_LT_ICMPV6_ECHO 132
#define GPK_LT_MLDV1_REPORT 135
#define GPK_LT_MLDV1_DONE 136
#define GPK_LT_MLDV1_QUERY 137
#define GPK_LT_MLDV2_REPORT 138
#define GPK_LT_MLDV2_QUERY 139

/* kinds mask of gpk_control_batch and gpk_control.kind */
#define GPK_CTL_ICMP4 1u
#define GPK_CTL_ICMP6 2u
#define GPK_CTL_ICMP6ECHO 4u
#define GPK_CTL_ARP 8u
#define GPK_CTL_ALL 15u

/* flags */
#define GPK_CTL_CSUM 1u /* VerifyChecksum of every ICMPv4 / ICMPv6 header that decoded */

/* verdict[i] of a packet that is not in the compact list */
#define GPK_CTL_NONE (-1)    /* not a candidate */
#define GPK_CTL_UNKNOWN (-2) /* decoded list longer than 16 entries */

/* classes of the compact list, in list order */
#define GPK_CTL_CLASS_ICMP4 0
#define GPK_CTL_CLASS_ICMP6 1  /* first layer ICMPv6, or ICMPv6Echo reached through a table edit */
#define GPK_CTL_CLASS_ARP 2
#define GPK_CTL_CLASS_FAILED 3 /* the first control layer's DecodeFromBytes returned an error */
#define GPK_CTL_NCLASS 4

/* gpk_control.err; gpk_control_format_error renders Go's text */
enum gpk_ctl_err {
  GPK_CTL_ERR_ICMP4_SHORT = 80, /* icmp4.go:224   "ICMP layer less then 8 bytes for ICMPv4 packet"  Truncated */
  GPK_CTL_ERR_ICMP6_SHORT = 81, /* icmp6.go:192   "ICMP layer less then 4 bytes for ICMPv6 packet"  Truncated */
  GPK_CTL_ERR_ECHO_SHORT = 82,  /* icmp6msg.go:158 "ICMP layer less then 4 bytes for ICMPv6 Echo"   Truncated */
  GPK_CTL_ERR_ARP_SHORT = 83,   /* arp.go:45      "ARP length %d too short" (a0)                    Truncated */
  GPK_CTL_ERR_ARP_EXPECTED = 84 /* arp.go:57      "ARP length %d too short, %d expected" (a0, a1)   Truncated */
};

/* gpk_control.status */
#define GPK_CTL_ST_TRUNCATED 1u /* a control layer called SetTruncated                          */
#define GPK_CTL_ST_CSUM 2u      /* the sum was made: `correct` holds Correct                     */
#define GPK_CTL_ST_VALID 4u     /* ... and Valid (correct == checksum; no zero exception)        */
#define GPK_CTL_ST_NONET 8u     /* ICMPv6 with GPK_CTL_CSUM and no network layer in the decoded
                                   list: computeChecksum returns its error (tcpip.go:55-57)      */

/* ---- one candidate (64 B) ----------------------------------------------------
 * Offsets are relative to the start of the packet. The fields describe the
 * FIRST control layer (kind); the layers the loop appended after it are named
 * in layer_types. When the first layer's decode fails (class FAILED), kind,
 * err, err_a0, err_a1, status and hdr_off are set and every other field is 0.
 * When ICMPv6 decoded and ICMPv6Echo after it failed, the record is the
 * ICMPv6's with nlayers 1 and err, err_a0, err_a1 and the Truncated bit the
 * Echo's.
 *
 * ARP: SourceHwAddress = packet[hdr_off + 8 : + hw], SourceProtAddress follows
 * for arp_prot_size bytes, then DstHwAddress and DstProtAddress (arp.go:59-62);
 * contents_len = 8 + 2 hw + 2 prot, the payload is the rest of the slice (the
 * padding of a 60-byte frame, since Ethernet trims 802.3 frames only).
 * ICMPv6Echo reached first through a table edit: kind GPK_CTL_ICMP6ECHO, id and
 * seq set, contents_len and payload_len 0 (it sets no BaseLayer). */
typedef struct gpk_control {
  uint8_t kind;           /*  0 GPK_CTL_* of the first control layer                          */
  uint8_t err;            /*  1 0 or gpk_ctl_err                                              */
  uint8_t status;         /*  2 GPK_CTL_ST_*                                                  */
  uint8_t nlayers;        /*  3 layers appended to the decoded list, 0..2                     */
  uint32_t err_a0;        /*  4                                                               */
  uint32_t err_a1;        /*  8                                                               */
  uint32_t hdr_off;       /* 12 packet offset of the first control layer's slice              */
  uint32_t contents_len;  /* 16 len(LayerContents())                                          */
  uint32_t payload_off;   /* 20 packet offset of LayerPayload()                               */
  uint32_t payload_len;   /* 24 len(LayerPayload())                                           */
  int32_t unsupported;    /* 28 the LayerType the loop returned for want of a decoder, 0: none */
  uint16_t layer_types[3];/* 32 LayerType of each appended layer, 0 past nlayers ([2] is 0)    */
  uint16_t typecode;      /* 38 ICMPv4.TypeCode / ICMPv6.TypeCode (type << 8 | code)          */
  uint16_t checksum;      /* 40 ICMPv4.Checksum / ICMPv6.Checksum                             */
  uint16_t correct;       /* 42 VerifyChecksum Correct when GPK_CTL_ST_CSUM                   */
  uint16_t id;            /* 44 ICMPv4.Id, or ICMPv6Echo.Identifier of the appended Echo      */
  uint16_t seq;           /* 46 ICMPv4.Seq, or ICMPv6Echo.SeqNumber                           */
  uint16_t arp_addr_type; /* 48 ARP.AddrType                                                  */
  uint16_t arp_protocol;  /* 50 ARP.Protocol                                                  */
  uint8_t arp_hw_size;    /* 52 ARP.HwAddressSize                                             */
  uint8_t arp_prot_size;  /* 53 ARP.ProtAddressSize                                           */
  uint16_t arp_operation; /* 54 ARP.Operation                                                 */
  int32_t next_type;      /* 56 NextLayerType() of the first control layer                    */
  uint32_t sum_init;      /* 60 ICMPv6 with a sum: computeChecksum's start value mod 2^32
                                (pseudo-header words + 58 + length & 0xffff + length >> 16)   */
} gpk_control;

/* Outputs, caller-allocated, n = batch size; m = counts[0] <= n entries are
 * written, nothing at or past m. The list is ordered by class and, inside a
 * class, by packet index. */
typedef struct gpk_controls {
  int32_t* verdict;      /* [n] position in the compact list, or GPK_CTL_NONE / GPK_CTL_UNKNOWN */
  uint32_t* class_start; /* [5] class c is entries [class_start[c], class_start[c+1])           */
  uint32_t* index;       /* [n] packet id of each entry                                         */
  gpk_control* records;  /* [n] 8-byte aligned                                                  */
  uint32_t* counts;      /* [8] m, the four class counts, sums made, 0, 0                       */
} gpk_controls;

typedef struct gpk_controller gpk_controller;

/* Workspace of the scans for batches of up to max_packets (< 2^28) on one
 * device. It serves one call at a time: calls on one stream are ordered,
 * concurrent streams need one controller each. */
int gpk_controller_create(gpk_controller** out, int device, uint64_t max_packets);
int gpk_controller_destroy(gpk_controller* c);

/* Decode the control layers at the end of a decoded batch. res holds the
 * records and layouts of gpk_decode_batch(ctx, parser, batch); every pointer is
 * device memory; batch->data is 16-byte aligned and readable up to the next
 * 16-byte boundary past its last packet; asynchronous on `stream`. kinds:
 * GPK_CTL_* mask of the layers the caller's parser holds; flags: GPK_CTL_CSUM.
 * GPK_EINVAL: a null argument, kinds 0 or outside GPK_CTL_ALL, unknown flags,
 * batch->n > max_packets, data not 16-byte aligned, records not 8-byte aligned. */
int gpk_control_batch(gpk_controller* c, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                      const gpk_results* res, uint32_t kinds, uint32_t flags, const gpk_controls* out, void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The decoders are the ones the kernels run. */
int gpk_control_batch_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                           uint32_t kinds, uint32_t flags, const gpk_controls* host_out);

/* The lane group of the sum: messages of at least `bytes` bytes are summed by
 * 64 lanes, shorter ones by 16 (default GPK_CTL_SUM_GROUP_BYTES, the GRE sum's
 * GPK_TUN_SUM_GROUP_BYTES). Results do not depend on it. */
#define GPK_CTL_SUM_GROUP_BYTES 8192
int gpk_controller_set_sum_threshold(gpk_controller* c, uint32_t bytes);

/* Go's error text of a gpk_control (err, err_a0, err_a1); as gpk_format_error. */
int gpk_control_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPK_CONTROL_H */
