/*
 * gpk_serialize.h — the writer half of the root package: gopacket.SerializeLayers
 * (writer.go:17-233) with the SerializeTo of the six hot-path layers, for the
 * packets of a device batch.
 *
 * A packet is serialized from three things: its source bytes, the gpk_layout the
 * decode produced for it, and a gpk_fields record (the decode's own, or one the
 * caller edited). Scalars come from the fields record. Variable-length parts
 * come from the source packet: IPv4 and TCP option bytes, the inline HopByHop
 * header and the payload; the option maps of the fields record say where the
 * options are. Nothing else is read; no gpk_record is needed.
 *
 * The layer list of one packet
 *   1. The slots k in {Ethernet, Dot1Q, IPv4, IPv6, TCP, UDP} whose layout slice
 *      is present, in ascending start.
 *   2. Each has a source Contents range [start, start + hdr), hdr read from the
 *      source bytes: Ethernet 14, Dot1Q 4, IPv4 IHL*4, IPv6 40 plus the inline
 *      HopByHop's ActualLength when NextHeader is 0 and the packet is not a
 *      jumbogram (ip6.go:239-263), TCP DataOffset*4, UDP 8.
 *   3. Walking the slots in that order: the source bytes between the previous
 *      Contents end and this start become a verbatim gopacket.Payload layer (the
 *      gap rule: a stacked layer's outer instance such as the outer QinQ tag or
 *      the outer header of IP in IP, or the IPv6 extension headers the skipper
 *      walked). The slot's own layer follows if its bit is still set in
 *      fields.present; a cleared bit drops that header (a VLAN pop clears the
 *      Dot1Q bit and sets eth_type = d1q_type).
 *   4. The tail is the innermost slot's LayerPayload() as its DecodeFromBytes
 *      leaves it: the IPv4 / IPv6 / UDP / 802.3 length trims apply
 *      (ip4.go:184-214, ip6.go:266-275, udp.go:44-55, ethernet.go:49-61); TCP and
 *      Dot1Q take the rest of their slice. A non-empty tail is the final Payload
 *      layer, so an Ethernet trailer is dropped; Ethernet.SerializeTo pads with
 *      zeros to 60 bytes (ethernet.go:95-103). A packet without any slot is its
 *      own bytes.
 *   5. The list is serialized innermost first, as SerializeLayers does
 *      (writer.go:207-218): a length field set by FixLengths counts what the
 *      inner layers wrote, and the first error is the innermost layer's.
 *
 * Harness rules (what a Go caller decides before calling SerializeLayers)
 *   - The pseudo-header of TCP / UDP (SetNetworkLayerForChecksum) is the
 *     serialized network layer with the greatest start. Its addresses are the
 *     fields record's, so an address rewrite reaches the L4 checksum. With
 *     ComputeChecksums and no network layer the status is the reference's error
 *     (tcpip.go:55-57).
 *   - TCP Padding, IPv4 Padding and the option lists come from this packet only.
 *   - PrependBytes leaves its bytes "indeterminate" (writer.go:88-92). They are
 *     zero here, as a fresh NewSerializeBuffer gives.
 *
 * Scope decisions
 *   - GPK_SER_ENOLAYER: a bit set in fields.present whose layout slice is absent.
 *     Inserting headers is not built.
 *   - GPK_SER_EHBHLONG: an inline HopByHop longer than 24 bytes, which the 24-bit
 *     option map cannot describe.
 *   - GPK_SER_EJUMBOADD: FixLengths on a payload over 65 535 bytes where the
 *     reference would insert a HopByHop header or a jumbo option
 *     (addIPv6JumboOption, ip6.go:80-102), or a padding option in front of an
 *     existing jumbo option that is off its 4n+2 alignment (ip6.go:374-390). An
 *     existing aligned 4-byte jumbo TLV is filled in as
 *     setIPv6PayloadJumboLength does (ip6.go:105-134).
 *   - GPK_SER_ELAYOUT: the layout or an option map does not describe this
 *     packet (a header that leaves its slice or the packet, slices that
 *     overlap, options that overlap or leave the packet), or a TCP / UDP slice
 *     that is not the innermost one (reachable only with edited port tables).
 *     Nothing outside the packet is ever read.
 *   - GPK_SER_EINDEX: order[j] is not a packet of the batch.
 *   These are checked first, in the order EINDEX, ENOLAYER, ELAYOUT; EHBHLONG
 *   and EJUMBOADD take the IPv6 layer's place in the innermost-first order.
 *
 * A packet in error writes nothing: out_caplens[j] == 0 and status[j] != 0.
 */
#ifndef GPK_SERIALIZE_H
#define GPK_SERIALIZE_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status[j]: 0, a reference error (> 0; its arguments in err_args[2j], [2j+1]),
 * or a scope code (< 0) */
#define GPK_SER_OK 0
#define GPK_SER_ERR_ETH_TYPE_LENGTH 1     /* a0=EthernetType a1=Length  "ethernet type %v not compatible with length value %v"  ethernet.go:87 */
#define GPK_SER_ERR_ETH_LENGTH 2          /* a0=Length  "invalid ethernet length %v"                                ethernet.go:89 */
#define GPK_SER_ERR_IP6_FIT_LEN 3         /* a0=length  "Cannot fit payload length of %d into IPv6 packet"          ip6.go:152 */
#define GPK_SER_ERR_IP6_JUMBO_MISSING 4   /* "Missing jumbo length hop-by-hop option"                               ip6.go:159 */
#define GPK_SER_ERR_IP6_JUMBO_TLV_LEN 5   /* "Jumbo length TLV data must have length 4"                             ip6.go:68  */
#define GPK_SER_ERR_IP6_JUMBO_SMALL 6     /* "Jumbo length cannot be less than 65536"                               ip6.go:72  */
#define GPK_SER_ERR_IP6_JUMBO_TLV_SHORT 7 /* a0=length  "Jumbo TLV too short (%d bytes)"                            ip6.go:129 */
#define GPK_SER_ERR_HBH_MULT8 8           /* "IPv6HopByHop actual length must be multiple of 8"                     ip6.go:494 */
#define GPK_SER_ERR_IP6_FIT 9             /* "Cannot fit payload into IPv6 header"                                  ip6.go:193 */
#define GPK_SER_ERR_L4_NO_NETWORK 10      /* "TCP/IP layer 4 checksum cannot be computed without network layer..."  tcpip.go:56 */
#define GPK_SER_ENOLAYER (-40)
#define GPK_SER_EHBHLONG (-41)
#define GPK_SER_EJUMBOADD (-42)
#define GPK_SER_EINDEX (-43)
#define GPK_SER_ELAYOUT (-44)

typedef struct gpk_serializer gpk_serializer;

/* device >= 0: the serializer owns the device workspace for calls of up to
 * max_packets output packets (< 2^31) on that device; it serves one call at a
 * time. device < 0: host only (no GPU is touched; gpk_serialize_batch returns
 * GPK_EINVAL). */
int gpk_serializer_create(gpk_serializer** out, int device, uint64_t max_packets);
int gpk_serializer_destroy(gpk_serializer* s);

/* gopacket.SerializeOptions */
typedef struct gpk_serialize_opts {
  uint32_t fix_lengths;
  uint32_t compute_checksums;
  uint32_t group; /* tests and measurements only: 0 = the library picks the move kernel's lanes per
                     packet from the batch's mean packet size; 16 or 64 force it */
} gpk_serialize_opts;

/* Serialize packets order[0..m) of a device batch (order NULL: packets 0..m-1;
 * repeats allowed). layouts and fields are indexed by SOURCE packet. Device
 * arrays:
 *   out         [out_cap], any alignment. Output packet j is out[out_offsets[j],
 *               out_offsets[j] + out_caplens[j]); the packets are packed back to
 *               back as gpk_pack_batch packs them, so {out, out_offsets,
 *               out_caplens, m} is a gpk_batch that decodes again. A packet that
 *               does not end inside out_cap is not written at all; nothing at or
 *               past out + out_cap is touched.
 *   out_offsets [m+1], out_caplens [m], status [m]
 *   err_args    [2m] or NULL; written only for packets in error
 *   counts      [4]  packets written, bytes needed (out_offsets[m]), packets in
 *               error, overflow (bytes needed > out_cap)
 * opts may be NULL (neither option, group 0). Asynchronous on `stream`; the
 * caller's HIP device is restored. Like the project's other byte movers it reads
 * whole aligned 16-byte words around a packet's bytes, so src->data must be one
 * allocation. */
int gpk_serialize_batch(gpk_serializer* s, const gpk_batch* src, const gpk_layout* layouts, const gpk_fields* fields,
                        const uint32_t* order, uint64_t m, const gpk_serialize_opts* opts, uint8_t* out,
                        uint64_t out_cap, uint64_t* out_offsets, uint32_t* out_caplens, int32_t* status,
                        uint32_t* err_args, uint64_t* counts, void* stream);
/* The same with host pointers, on the calling thread. */
int gpk_serialize_batch_host(gpk_serializer* s, const gpk_batch* src, const gpk_layout* layouts,
                             const gpk_fields* fields, const uint32_t* order, uint64_t m,
                             const gpk_serialize_opts* opts, uint8_t* out, uint64_t out_cap, uint64_t* out_offsets,
                             uint32_t* out_caplens, int32_t* status, uint32_t* err_args, uint64_t* counts);

/* The reference's text of a positive status, as gpk_format_error renders decode
 * errors. Returns the length written (without the NUL), 0 for a status that is
 * not a reference error. The EthernetType of GPK_SER_ERR_ETH_TYPE_LENGTH is
 * rendered as its number; a caller with the reference's names substitutes it. */
int gpk_serialize_format_error(int status, uint32_t a0, uint32_t a1, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GPK_SERIALIZE_H */
