/*
 * gpk_svc.h — decode the UDP service layers DHCPv4, DHCPv6 and NTP on the
 * device.
 *
 * UDPPort.LayerType() (layers/ports.go:121-170) leads to LayerTypeDHCPv4 (ports
 * 67, 68), LayerTypeNTP (123) and LayerTypeDHCPv6 (546, 547). A Go caller adds
 * &layers.DHCPv4{}, &layers.DHCPv6{} and &layers.NTP{} to its
 * DecodingLayerParser. This entry group is that step for a decoded batch: for
 * every packet whose decode ends in front of one of them it runs the layer's
 * DecodeFromBytes (layers/dhcpv4.go:126-184, 563-583, dhcpv6.go:89-124,
 * dhcpv6_options.go:611-622, ntp.go:294-347). The two DHCPs are a fixed head
 * plus an option list, so the result is not a fixed-size record: the message
 * record (gpk_svc) names a range of 8-byte entries (gpk_svc_entry), one per
 * option. Addresses, names and option bytes stay in the packet: the arena
 * holds descriptors only. The kinds mask leaves room for further UDP services.
 *
 * Rules
 *   Candidate   tun::candidate of gpk_tunnel.h, unchanged: the last decoded
 *               layer's NextLayerType(), recomputed from its gpk_layout slot
 *               and the parser's tables, is an enabled kind; the message is
 *               that layer's payload and it is not empty. So the UDP
 *               destination port counts before the source port
 *               (layers/udp.go NextLayerType), RegisterUDPPortLayerType edits,
 *               a TCP port or EtherType the caller pointed at one of the three
 *               and ignore_unsupported count. A decoded list longer than 16
 *               entries gives GPK_SVC_UNKNOWN.
 *   Loop        Every one of the three ends the reference's loop
 *               (layers_decoder.go:60-79) with nil: DHCPv4 and DHCPv6 answer
 *               LayerTypePayload but never set Payload, so the loop stops on
 *               the empty payload (:71); NTP answers LayerTypeZero with an
 *               empty payload. The composed list gains exactly one layer type
 *               and the composed error becomes nil; on a failure nothing is
 *               appended and the error is the message's.
 *   DHCPv4      dhcpv4.go:126-184. len < 240: "DHCPv4 length %d too short",
 *               Truncated. HardwareLen (data[2]) > 16: "DHCPv4 hardware address
 *               length %d exceeds 16", not Truncated. data[236:240] is not
 *               0x63825363: "Bad DHCP header". len == 240: nil, no options, and
 *               Contents is NOT set (:155-158 return in front of :181):
 *               contents_len is 0. Otherwise the loop over data[240:] with
 *               DHCPOption.decode (:563-583): Pad (0) is one byte and IS
 *               appended (Length 0, no Data); End (255) stops the loop, is not
 *               appended, and the bytes behind it are ignored; any other type
 *               at the last byte: "Not enough data to decode"; Length greater
 *               than the bytes left behind the two: "Option is malformed";
 *               neither sets Truncated. The loop also ends, without an End,
 *               where the data does. Contents = data only after the loop.
 *   DHCPv6      dhcpv6.go:89-124. len < 4: "DHCPv6 length %d too short",
 *               Truncated. MsgType 12 or 13 (relay) with len < 34: "DHCPv6
 *               length %d too short for message type %d", Truncated. Options
 *               start at 34 for a relay message, else at 4, and run to the end
 *               of the data with DHCPv6Option.decode (dhcpv6_options.go:
 *               611-622): fewer than 4 bytes left: "not enough data to decode";
 *               fewer than 4 + int(Length): "dhcpv6 option size < length %d",
 *               where the printed value is 4 + o.Length computed in uint16: a
 *               Length of 0xFFFC..0xFFFF prints 0..3. Neither sets Truncated.
 *               Contents = data is set in front of the loop: every successful
 *               message has contents_len == len.
 *   NTP         ntp.go:294-347. len < 48: "NTP packet too short", Truncated.
 *               Otherwise Contents = data and ExtensionBytes = data[48:].
 *   Guarded     Every slice expression of the three paths, for a run-time
 *               panic. DHCPv4: data[a:b] of the head sit behind len >= 240;
 *               data[28 : 28+HardwareLen] is a uint8 sum, but HardwareLen <= 16
 *               is checked in front, so it neither wraps nor passes 44;
 *               options[start:] has start <= stop because an option's 2 +
 *               Length never exceeds what decode was handed; data[2:] has
 *               len >= 2; data[2 : 2+int(Length)] is an int sum behind its
 *               guard. NTP: all behind len >= 48. DHCPv6: data[offset:] is
 *               guarded the same way, but ONE expression is not:
 *               data[4 : 4+o.Length] (dhcpv6_options.go:620) adds in uint16
 *               while its guard (:617) adds in int. For a Length of
 *               0xFFFC..0xFFFF with at least 4 + Length (65 536..65 539) bytes
 *               left the guard passes and the high bound wraps to h = 0..3,
 *               below the low bound: Go panics with "slice bounds out of range
 *               [4:h]", which DecodeLayers turns into an error. A UDP payload
 *               cannot be that long, but the payload of a layer a table edit
 *               points at one of the three (an EtherType, a TCP port) can.
 *               Reported as GPK_ERR_PANIC_SLICE_B (gpk.h), a0 = 4, a1 = h, not
 *               Truncated. A shorter rest takes the guarded error above.
 *
 * Scope decisions
 *   Fresh struct  Every message is decoded into a fresh struct. The reference's
 *               DHCPv4 keeps an earlier packet's Contents when a reused struct
 *               decodes a 240-byte message or fails early, and all three keep
 *               the fields an early return did not reach. Here a message's
 *               fields are its own: contents_len of a 240-byte DHCPv4 is 0.
 *   Failed      A failed message has no entries and no scalars: the options
 *               the reference had appended in front of the error and the head
 *               fields it had stored are not reported.
 *   Timestamps  The four 64-bit NTP timestamps are not copied into the record:
 *               they are the 32 bytes at packet offset hdr_off + 16 (Reference,
 *               Origin, Receive, Transmit; big-endian). The record stays 64
 *               bytes for all three layers.
 */
#ifndef GPK_SVC_H
#define GPK_SVC_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_LT_NTP 117
#define GPK_LT_DHCPV4 118
#define GPK_LT_DHCPV6 134

/* kinds mask of gpk_svc_batch: the layers the caller's parser holds */
#define GPK_SVC_DHCP4 1u /* layers.DHCPv4 */
#define GPK_SVC_DHCP6 2u /* layers.DHCPv6 */
#define GPK_SVC_NTP 4u   /* layers.NTP    */
#define GPK_SVC_ALL 7u

/* verdict[i] of a packet that is not in the compact list */
#define GPK_SVC_NONE (-1)    /* not a candidate */
#define GPK_SVC_UNKNOWN (-2) /* decoded list longer than 16 entries */

/* classes of the compact list, in list order */
#define GPK_SVC_CLASS_OK 0
#define GPK_SVC_CLASS_FAILED 1 /* DecodeFromBytes returned an error or panicked */
#define GPK_SVC_NCLASS 2

/* gpk_svc.err: one of these or GPK_ERR_PANIC_SLICE_B (gpk.h); gpk_svc_format_error renders Go's text */
enum gpk_svc_err {
  GPK_SVC_ERR_DHCP4_SHORT = 160,  /* dhcpv4.go:129 "DHCPv4 length %d too short" (a0 len)                  Truncated */
  GPK_SVC_ERR_DHCP4_HLEN,         /* :138 "DHCPv4 hardware address length %d exceeds 16" (a0 HardwareLen)           */
  GPK_SVC_ERR_DHCP4_MAGIC,        /* :152, :599 "Bad DHCP header"                                                   */
  GPK_SVC_ERR_DHCP4_OPT_SHORT,    /* :574, :595 "Not enough data to decode"                                         */
  GPK_SVC_ERR_DHCP4_OPT_MALFORMED,/* :578, :597 "Option is malformed"                                               */
  GPK_SVC_ERR_DHCP6_SHORT,        /* dhcpv6.go:92 "DHCPv6 length %d too short" (a0 len)                   Truncated */
  GPK_SVC_ERR_DHCP6_RELAY_SHORT,  /* :102 "DHCPv6 length %d too short for message type %d" (a0 len, a1)   Truncated */
  GPK_SVC_ERR_DHCP6_OPT_SHORT,    /* dhcpv6_options.go:613 "not enough data to decode"                              */
  GPK_SVC_ERR_DHCP6_OPT_LENGTH,   /* :618 "dhcpv6 option size < length %d" (a0 = uint16(4 + Length))                */
  GPK_SVC_ERR_NTP_SHORT,          /* ntp.go:299 "NTP packet too short"                                    Truncated */
  GPK_SVC_ERR_END
};

/* gpk_svc.status */
#define GPK_SVC_ST_TRUNCATED 1u /* DecodeFromBytes called SetTruncated                                    */
#define GPK_SVC_ST_DROPPED 2u   /* the message decoded, but its entries did not fit entry_cap: none written */

/* ---- one candidate (64 B) ----------------------------------------------------
 * Offsets are relative to the start of the packet; the message is
 * packet[hdr_off : hdr_off + len]. contents_len is len(LayerContents()): len,
 * but 0 for a DHCPv4 message of exactly 240 bytes. LayerPayload() is empty for
 * all three. The message's entries are entries[entry0 .. entry0 + nentries),
 * its options; entry0 is the sum of nentries of the entries in front of it in
 * the compact list, whether those fitted or not. b[] and v[] by layer type (0
 * where unused):
 *   DHCPv4  b: Operation, HardwareType (the low 8 bits LinkType holds), HardwareLen,
 *           RelayHops. v0 Xid, v1 Secs | Flags << 16, v2..v5 ClientIP,
 *           YourClientIP, NextServerIP, RelayAgentIP by value: bytes 48..63 of
 *           the record are data[12:28] in packet order. ClientHWAddr is the
 *           HardwareLen bytes at hdr_off + 28, ServerName the 64 at hdr_off +
 *           44, File the 128 at hdr_off + 108.
 *   DHCPv6  b: MsgType, HopCount (relay), 0, 0. A relay message (MsgType 12,
 *           13): v1 packet offset of LinkAddr (hdr_off + 2), v2 of PeerAddr
 *           (hdr_off + 18), 16 bytes each. Any other: v0 the three
 *           TransactionID bytes data[1:4] as a big-endian number.
 *   NTP     b: LeapIndicator, Version, Mode, Stratum. v0 Poll | Precision << 8
 *           (each the raw byte of an int8), v1 RootDelay, v2 RootDispersion, v3
 *           ReferenceID, v4 packet offset of ExtensionBytes (hdr_off + 48), v5
 *           their length (len - 48). The timestamps: see "Timestamps" above.
 * A failed message (class FAILED) has layer_type, err, err_a0, err_a1, status
 * and hdr_off set and every other field 0: no entries. */
typedef struct gpk_svc {
  uint8_t layer_type;    /*  0 GPK_LT_NTP, GPK_LT_DHCPV4 or GPK_LT_DHCPV6        */
  uint8_t err;           /*  1 0, gpk_svc_err or GPK_ERR_PANIC_SLICE_B           */
  uint8_t status;        /*  2 GPK_SVC_ST_*                                      */
  uint8_t reserved;      /*  3 0                                                 */
  uint32_t err_a0;       /*  4                                                   */
  uint32_t err_a1;       /*  8                                                   */
  uint32_t hdr_off;      /* 12 packet offset of the message                      */
  uint32_t len;          /* 16 its length                                        */
  uint32_t contents_len; /* 20 len(LayerContents())                              */
  uint64_t entry0;       /* 24 first entry in entries                            */
  uint32_t nentries;     /* 32 options                                           */
  uint8_t b[4];          /* 36 the layer's byte scalars                          */
  uint32_t v[6];         /* 40 the layer's scalars, addresses and offsets        */
} gpk_svc;

/* ---- one option (8 B) -----------------------------------------------------------
 * DHCPOption: code is Type, length Length (0 for a Pad). DHCPv6Option: code
 * is Code, length Length. off is the packet offset of Data (length bytes; for a
 * Pad the offset behind its one byte). */
typedef struct gpk_svc_entry {
  uint16_t code;   /* 0 */
  uint16_t length; /* 2 */
  uint32_t off;    /* 4 */
} gpk_svc_entry;

/* Outputs, caller-allocated, n = batch size; m = counts[0] <= n entries of
 * index and records are written, nothing at or past m. The list is ordered by
 * class and, inside a class, by packet index. entries holds entry_cap
 * entries; nothing is written at or past it. A message's entries are written
 * only when its whole range fits (entry0 + nentries <= entry_cap); otherwise
 * its record carries GPK_SVC_ST_DROPPED. counts tells what a retry needs. */
typedef struct gpk_svcs {
  int32_t* verdict;       /* [n] position in the compact list, or GPK_SVC_NONE / GPK_SVC_UNKNOWN */
  uint32_t* class_start;  /* [3] class c is entries [class_start[c], class_start[c+1])           */
  uint32_t* index;        /* [n] packet id of each entry                                         */
  gpk_svc* records;       /* [n] 8-byte aligned                                                  */
  uint32_t* counts;       /* [8] m, OK, FAILED, overflow (1: something was dropped), entries
                                 needed (low, high dword), 0, 0                                   */
  gpk_svc_entry* entries; /* [entry_cap] 8-byte aligned; may be null when entry_cap is 0         */
  uint64_t entry_cap;
} gpk_svcs;

typedef struct gpk_svc_decoder gpk_svc_decoder;

/* Workspace of the scans for batches of up to max_packets (< 2^28) on one
 * device. It serves one call at a time: calls on one stream are ordered,
 * concurrent streams need one decoder each. */
int gpk_svc_decoder_create(gpk_svc_decoder** out, int device, uint64_t max_packets);
int gpk_svc_decoder_destroy(gpk_svc_decoder* d);

/* Work per message is linear in its length. One lane walks a message, three
 * times: in the classify and the scatter step (counting) and in the emit
 * step. A DHCPv6 option takes at least 4 bytes and a DHCPv4 option 2, but a
 * DHCPv4 Pad is an entry of one byte: the worst case is a DHCPv4 message of
 * Pad bytes, one step and one 8-byte entry per byte (a 1 500-byte frame: about
 * 1 200 entries, 9.6 KB). NTP is constant. Nothing is super-linear.
 *
 * Decode the DHCPv4, DHCPv6 and NTP messages at the end of a decoded batch.
 * res holds the records and layouts of gpk_decode_batch(ctx, parser, batch);
 * every pointer is device memory; batch->data is 16-byte aligned; asynchronous
 * on `stream`; the caller's HIP device is restored. kinds: GPK_SVC_* mask of
 * the layers the caller's parser holds. GPK_EINVAL: a null argument, kinds 0 or
 * outside GPK_SVC_ALL, batch->n > max_packets, data not 16-byte aligned,
 * records or entries not 8-byte aligned, entries null with entry_cap > 0. */
int gpk_svc_batch(gpk_svc_decoder* d, gpk_ctx* ctx, const gpk_parser* parser, const gpk_batch* batch,
                  const gpk_results* res, uint32_t kinds, const gpk_svcs* out, void* stream);

/* The same outputs from host arrays, on the calling thread; no GPU is touched.
 * The walk is the one the kernels run. */
int gpk_svc_batch_host(const gpk_parser* parser, const gpk_batch* host_batch, const gpk_results* host_res,
                       uint32_t kinds, const gpk_svcs* host_out);

/* Go's error text of a gpk_svc (err, err_a0, err_a1); as gpk_format_error. */
int gpk_svc_format_error(unsigned err, uint32_t a0, uint32_t a1, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPK_SVC_H */
