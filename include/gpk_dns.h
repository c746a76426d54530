/*
 * gpk_dns.h — decode the DNS messages of a decoded batch on the device
 * (DESIGN.md §23).
 *
 * UDP and TCP port 53 lead to LayerTypeDNS (107) in the port tables
 * (layers/ports.go:59-60,126-127) and the parser has no decoder for it. A Go
 * caller adds &layers.DNS{} to its DecodingLayerParser. This entry group is
 * that step for a decoded batch: for every packet whose decoded list ends in
 * front of LayerTypeDNS it runs DNS.DecodeFromBytes (layers/dns.go:333-421).
 * The result is not a fixed-size record: the message record (gpk_dns) names a
 * range of entry records (gpk_dns_rr, one per question or resource record)
 * and a range of a byte arena that holds the decoded names.
 *
 * Rules
 *   Candidate   tun::candidate, unchanged (gpk_tunnel.h): the NextLayerType()
 *               of the last layer of the decoded list, recomputed from its
 *               gpk_layout slot with the parser's tables, is 107 and that
 *               layer's LayerPayload() is not empty. Table edits count:
 *               RegisterTCPPortLayerType(8080, LayerTypeDNS) makes 8080 a DNS
 *               port. A decoded list longer than 16 entries gives
 *               GPK_DNS_UNKNOWN.
 *   Slice       data is that payload. Over TCP it starts with the two length
 *               bytes, which the reference decodes as the ID (decodeDNS is
 *               the same function for both, dns.go:321-330); so does this.
 *               gpk_dns_streams.h frames the messages of reassembled TCP
 *               streams by those bytes and decodes each one whole.
 *   Loop        DNS sets BaseLayer{Contents: data} only and Payload() returns
 *               nil (dns.go:343,434-436): the reference's loop ends after it
 *               with nil. 107 is appended to the decoded list, nothing follows.
 *   Message     The 12 header bytes; QDCount questions (dns.go:933-952);
 *               ANCount, NSCount, ARCount records (:1056-1087), each with
 *               decodeRData over data[:end] (:1350-1529), end being the
 *               record's end: a pointer inside RDATA cannot reach past it. A
 *               record with DataLength 0 skips decodeRData. ResponseCode
 *               takes the extended RCODE of every additional OPT record,
 *               uint8(rc) | uint8(TTL>>20 & 0xF0), cumulatively (:406-408).
 *   Name        decodeName (dns.go:814-920), iteratively: a pointer ends its
 *               level (break loop), so the recursion is a tail call. Its
 *               checks, in its order, with `offset` the level's own start:
 *               level > 255; offset >= len; a first zero byte returns at
 *               once; per label index2 - offset > 255, then index2 > len;
 *               per pointer index + 2 > len, then offsetp > len (offsetp ==
 *               len passes and fails the next level's offset >= len); the
 *               0x40 and 0x80 forms with data[index] and index in the text;
 *               index >= len after a label. The name is the labels' raw
 *               bytes joined by '.', no leading dot, no escaping; a name that
 *               is only a pointer to the root is empty.
 *   RRSIG       decodes its signer into its own buffer and strips one leading
 *               '.' only when the buffer is longer than 1 (dns.go:1739-1742).
 *               A decoded name's buffer is empty or '.' plus a label of at
 *               least one byte, so the result is the same join.
 *   Labels      dnsNameMeta / collectDNSWireLabels serve SerializeTo only and
 *               are not part of the result.
 *   Unreachable errDecodeQueryBad*Count (the loops append exactly the counts),
 *               errDNSNameOffsetNegative (offsets are sums of non-negative
 *               terms), "DNSSVCB record is empty" and decodeOPTs' empty return
 *               (decodeRData runs for DataLength > 0 only). No slice
 *               expression of the path is unguarded: there is no run-time
 *               panic to report.
 */
#ifndef GPK_DNS_H
#define GPK_DNS_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_LT_DNS 107

/* kinds mask of gpk_dns_batch and gpk_dns.kind */
#define GPK_DNS_KIND 1u
#define GPK_DNS_ALL 1u

/* verdict[i] of a packet that is not in the compact list */
#define GPK_DNS_NONE (-1)    /* not a candidate */
#define GPK_DNS_UNKNOWN (-2) /* decoded list longer than 16 entries */

/* classes of the compact list, in list order */
#define GPK_DNS_CLASS_OK 0
#define GPK_DNS_CLASS_FAILED 1 /* DecodeFromBytes returned an error */
#define GPK_DNS_NCLASS 2

/* gpk_dns.err; gpk_dns_format_error renders Go's text */
enum gpk_dns_err {
  GPK_DNS_ERR_SHORT = 90,        /* :338  "DNS packet too short"                      Truncated */
  GPK_DNS_ERR_MAX_RECURSION,     /* :816  "max DNS recursion level hit"                         */
  GPK_DNS_ERR_OFFSET_HIGH,       /* :818  "dns name offset too high"                            */
  GPK_DNS_ERR_NAME_LONG,         /* :842  "dns name is too long"                                */
  GPK_DNS_ERR_INVALID_INDEX,     /* :844  "dns name uncomputable: invalid index"                */
  GPK_DNS_ERR_POINTER_HIGH,      /* :877,:881 "dns offset pointer too high"                     */
  GPK_DNS_ERR_INDEX_RANGE,       /* :913  "dns index walked out of range"                       */
  GPK_DNS_ERR_QNAME40,           /* :905  "qname '0x40' - RFC 2673 unsupported yet (data=%x index=%d)"
                                          (a0, a1)                                               */
  GPK_DNS_ERR_QNAME80,           /* :909  "qname '0x80' unsupported yet (data=%x index=%d)" (a0, a1) */
  GPK_DNS_ERR_QUESTION_SMALL,    /* :940  "DNS question too small"                              */
  GPK_DNS_ERR_RECORD_SMALL,      /* :1063 "DNS record too small"                                */
  GPK_DNS_ERR_RECORD_LENGTH,     /* :1076 "resource record length exceeds data"                 */
  GPK_DNS_ERR_CHARSTRING,        /* :1273 "Insufficient data for a <character-string>"          */
  GPK_DNS_ERR_SOA_SMALL,         /* :1404 "SOA too small"                                       */
  GPK_DNS_ERR_MX_SMALL,          /* :1417 "MX too small"                                        */
  GPK_DNS_ERR_URI_SMALL,         /* :1430 "URI too small"                                       */
  GPK_DNS_ERR_SRV_SMALL,         /* :1437 "SRV too small"                                       */
  GPK_DNS_ERR_NAPTR_SMALL,       /* :1452 "NAPTR too small"                                     */
  GPK_DNS_ERR_NAPTR_FLAGS_MISSING,   /* :1459 "NAPTR Flags missing"                             */
  GPK_DNS_ERR_NAPTR_FLAGS_TRUNC,     /* :1464 "NAPTR Flags truncated"                           */
  GPK_DNS_ERR_NAPTR_SERVICE_MISSING, /* :1470 "NAPTR Service missing"                           */
  GPK_DNS_ERR_NAPTR_SERVICE_TRUNC,   /* :1475 "NAPTR Service truncated"                         */
  GPK_DNS_ERR_NAPTR_REGEXP_MISSING,  /* :1481 "NAPTR Regexp missing"                            */
  GPK_DNS_ERR_NAPTR_REGEXP_TRUNC,    /* :1486 "NAPTR Regexp truncated"                          */
  GPK_DNS_ERR_OPT_LENGTH,        /* :1289 "DNSOPT record is of length %d, it should be at least length 4" (a0) */
  GPK_DNS_ERR_OPT_MALFORMED,     /* :1295 "Malformed DNSOPT record.  Length %d < %d" (a0, a1)   */
  GPK_DNS_ERR_OPT_IMPLIES,       /* :1300 "Malformed DNSOPT record. The length (%d) field implies a packet
                                          larger than the one received" (a0)                     */
  GPK_DNS_ERR_SVCB_LENGTH,       /* :1318 "DNSSVCB record is of length %d, it should be at least length 3" (a0) */
  GPK_DNS_ERR_SVCB_TRUNC,        /* :1329,:1334 "DNSSVCB record truncated in SvcParams"         */
  GPK_DNS_ERR_RRSIG_SMALL,       /* :1728 "RRSIG too small"                                     */
  GPK_DNS_ERR_DNSKEY_SMALL,      /* :1817 "DNSKEY too small"                                    */
  GPK_DNS_ERR_END
};

/* gpk_dns.status */
#define GPK_DNS_ST_TRUNCATED 1u /* DecodeFromBytes called SetTruncated ("DNS packet too short" only) */
#define GPK_DNS_ST_DROPPED 2u   /* the message decoded, but its entries or names did not fit
                                   rr_cap / name_cap: neither was written                         */

/* ---- one candidate (64 B) ----------------------------------------------------
 * hdr_off is relative to the start of the packet; the message is
 * packet[hdr_off : hdr_off + len] (BaseLayer.Contents). From the two raw flag
 * bytes: QR = flags2 & 0x80, OpCode = flags2 >> 3 & 0xF, AA = flags2 & 4,
 * TC = flags2 & 2, RD = flags2 & 1, RA = flags3 & 0x80, Z = flags3 >> 4 & 7
 * (dns.go:345-351). response_code is flags3 & 0xF or-ed with the OPT
 * extension. The message's entries are rrs[rr0 .. rr0 + nrr): questions, then
 * answers, authorities and additionals, in message order; its names are
 * names[name0 .. name0 + name_bytes). rr0 and name0 are the sums of nrr and
 * name_bytes of the OK entries in front of it, whether those fitted or not.
 * A failed message (class FAILED) has kind, err, err_a0, err_a1, status and
 * hdr_off set and every other field 0: no entries, no names. */
typedef struct gpk_dns {
  uint8_t kind;          /*  0 GPK_DNS_KIND                                     */
  uint8_t err;           /*  1 0 or gpk_dns_err                                 */
  uint8_t status;        /*  2 GPK_DNS_ST_*                                     */
  uint8_t response_code; /*  3 DNS.ResponseCode                                 */
  uint32_t err_a0;       /*  4                                                  */
  uint32_t err_a1;       /*  8                                                  */
  uint32_t hdr_off;      /* 12 packet offset of the message                     */
  uint32_t len;          /* 16 len(Contents)                                    */
  uint16_t id;           /* 20 DNS.ID                                           */
  uint8_t flags2;        /* 22 data[2]                                          */
  uint8_t flags3;        /* 23 data[3]                                          */
  uint16_t qdcount;      /* 24 */
  uint16_t ancount;      /* 26 */
  uint16_t nscount;      /* 28 */
  uint16_t arcount;      /* 30 */
  uint32_t nrr;          /* 32 questions + records                              */
  uint32_t reserved;     /* 36 0                                                */
  uint64_t rr0;          /* 40 first entry in rrs                               */
  uint64_t name0;        /* 48 first byte in names                              */
  uint64_t name_bytes;   /* 56 bytes of all its names                           */
} gpk_dns;

/* section of an entry */
#define GPK_DNS_SEC_QUESTION 0
#define GPK_DNS_SEC_ANSWER 1
#define GPK_DNS_SEC_AUTHORITY 2
#define GPK_DNS_SEC_ADDITIONAL 3

/* ---- one question or resource record (96 B) ------------------------------------
 * Offsets named *_off into the packet are relative to the start of the packet
 * (not of the message); name ranges are absolute positions in the name arena.
 * A question has section, type, class and the name range; the rest is 0.
 * Data = packet[data_off : data_off + data_length]; IP (A, AAAA) and TXT are
 * Data. rname: NS, CNAME, PTR, MX.Name, SRV.Name, SOA.MName,
 * NAPTR.Replacement, SVCB.Target, RRSIG.SignerName; rname2: SOA.RName.
 * v[] by type (0 where unused):
 *   MX      v0 Preference
 *   SRV     v0 Priority, v1 Weight, v2 Port
 *   URI     v0 Priority, v1 Weight; Target = Data[4:]
 *   SOA     v0 Serial, v1 Refresh, v2 Retry, v3 Expire, v4 Minimum
 *   NAPTR   v0 Order, v1 Preference, v2/v3 packet offset and length of Flags,
 *           v4/v5 of Service, v6/v7 of Regexp
 *   RRSIG   v0 TypeCovered, v1 Algorithm, v2 Labels, v3 OriginalTTL,
 *           v4 Expiration, v5 Inception, v6 KeyTag, v7/v8 packet offset and
 *           length of Signature
 *   DNSKEY  v0 Flags, v1 Protocol, v2 Algorithm; PublicKey = Data[4:]
 *   SVCB / HTTPS
 *           v0 Priority, v1 packet offset of the first SvcParam (they run to
 *           the end of Data)
 * count: the character-strings of TXT / HINFO (a walk over Data, each one
 * length byte then the bytes), the options of OPT (over Data: code, length,
 * bytes) or the SvcParams (from v1: key, length, bytes). The device has
 * validated the walk. */
typedef struct gpk_dns_rr {
  uint8_t section;      /*  0 GPK_DNS_SEC_*                 */
  uint8_t reserved;     /*  1 0                             */
  uint16_t type;        /*  2 DNSType                       */
  uint16_t cls;         /*  4 DNSClass                      */
  uint16_t data_length; /*  6 DataLength                    */
  uint32_t ttl;         /*  8 TTL                           */
  uint32_t data_off;    /* 12 packet offset of Data         */
  uint64_t name_off;    /* 16 Name in the arena             */
  uint32_t name_len;    /* 24                               */
  uint32_t count;       /* 28                               */
  uint64_t rname_off;   /* 32 first RDATA name              */
  uint32_t rname_len;   /* 40                               */
  uint32_t rname2_len;  /* 44                               */
  uint64_t rname2_off;  /* 48 second RDATA name (SOA.RName) */
  uint32_t v[10];       /* 56 the typed form's scalars      */
} gpk_dns_rr;

/* Outputs, caller-allocated, n = batch size; m = counts[0] <= n entries of
 * index and records are written, nothing at or past m. The list is ordered by
 * class and, inside a class, by packet index. rrs holds rr_cap entries and
 * names name_cap bytes; nothing is written at or past either. A message's
 * entries and names are written only when its whole range fits both
 * capacities (rr0 + nrr <= rr_cap and name0 + name_bytes <= name_cap);
 * otherwise its record carries GPK_DNS_ST_DROPPED. counts tells what a retry
 * needs. */
typedef struct gpk_dnss {
  int32_t* verdict;      /* [n] position in the compact list, or GPK_DNS_NONE / GPK_DNS_UNKNOWN */
  uint32_t* class_start; /* [3] class c is entries [class_start[c], class_start[c+1])           */
  uint32_t* index;       /* [n] packet id of each entry                                         */
  gpk_dns* records;      /* [n] 8-byte aligned                                                  */
  uint32_t* counts;      /* [8] m, OK, FAILED, overflow (1: something was dropped), entries
                                needed (low, high dword), name bytes needed (low, high)          */
  gpk_dns_rr* rrs;       /* [rr_cap] 8-byte aligned; may be null when rr_cap is 0               */
  uint8_t* names;        /* [name_cap] may be null when name_cap is 0                           */
  uint64_t rr_cap;
  uint64_t name_cap;
} gpk_dnss;

typedef struct gpk_dns_decoder gpk_dns_decoder;

/* Workspace of the scans for batches of up to max_packets (< 2^28) on one
 * device. It serves one call at a time: calls on one stream are ordered,
 * concurrent streams need one decoder each. */
int gpk_dns_decoder_create(gpk_dns_decoder** out, int device, uint64_t max_packets);
int gpk_dns_decoder_destroy(gpk_dns_decoder* d);

/* Work per message. One lane walks a message, three times: in the classify
 * and the scatter step (sizes only) and in the emit step. A name costs at most
 * 255 levels of at most 127 labels, and a message of len bytes holds at most
 * len / 5 names, so the bound is len / 5 x 32 385 label steps; what a crafted
 * message reaches is about len^2 / 100 steps (half of it label runs chained by
 * pointers, half of it records whose names point at them), each a dependent
 * byte load of roughly 0.4 us on an MI355X. At 1500 bytes that is some ten
 * thousand steps (12 ms for 1 Ki messages of 8 203 steps
 * that decode, 24 ms for 1 Ki failing loops of 32 130); at a
 * 64 KiB capture record it is tens of millions, seconds in one lane. The
 * reference pays the same steps on a CPU. The pass does not cap them, since a
 * cap would change results: a caller that decodes untrusted traffic on a
 * shared device bounds caplen (the snap length) of the batches it hands in.
 *
 * Decode the DNS messages at the end of a decoded batch. res holds the records
 * and layouts of gpk_decode_batch(ctx, parser, batch); every pointer is device
 * memory; batch->data is 16-byte aligned; asynchronous on `stream`; the
 * caller's HIP device is restored. GPK_EINVAL: a null argument, batch->n >
 * max_packets, data not 16-byte aligned, records or rrs not 8-byte aligned,
 * rrs null with rr_cap > 0, names null with name_cap > 0. */
int gpk_dns_batch(gpk_dns_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                  const gpk_results* res, const gpk_dnss* out, void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The walk is the one the kernels run. */
int gpk_dns_batch_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                       const gpk_dnss* host_out);

/* Go's error text of a gpk_dns (err, err_a0, err_a1); as gpk_format_error. */
int gpk_dns_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPK_DNS_H */
