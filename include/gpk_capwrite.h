/*
 * gpk_capwrite.h — the writer half of pcapgo: pcapgo.Writer (pcapgo/write.go)
 * and pcapgo.NgWriter (pcapgo/ngwrite.go, ngwrite_dsb.go), with the packets of
 * a device batch framed on the device.
 *
 * A gpk_capwriter holds what the reference's writer objects hold: the format
 * and, for pcapng, the number of interfaces added so far. It owns no file: every
 * function writes bytes into a caller buffer, and the caller appends them to its
 * file in call order. Everything is little endian, as the reference writes.
 *
 * The blocks that are not packets (file header, section header, interface
 * description, interface statistics, decryption secrets) are built on the host.
 * Each builder returns the block's length in bytes (> 0); when that exceeds
 * `cap` nothing is written and nothing is counted, and the caller repeats the
 * call with a larger buffer. A negative return is a GPK_E* or GPK_CAPW_E* code.
 *
 * The packets are framed by gpk_capwrite_batch (device) or
 * gpk_capwrite_batch_host (the same arguments as host pointers, on the CPU:
 * single-packet WritePacket and the CPU baseline). Output j is what one
 * WritePacket(ci[i], data_i) call with i = order[j] would have handed its
 * io.Writer:
 *   pcapng (ngwrite.go:361-411)  a 28-byte head {6, length, uint32(iface),
 *       uint32(ts >> 32), uint32(ts), caplen, ci.length}, ts = ts_sec * 1e9 +
 *       ts_nsec as a wrapping int64 (Time.UnixNano), so pre-1970 and zero times
 *       come out as Go writes them; the data; zero padding to a multiple of 4;
 *       the packet's option bytes as given; the length again.
 *   pcap (write.go:101-129)      {uint32(ts_sec), ts_nsec / 1000 (microsecond
 *       format) or ts_nsec (nanosecond format), caplen, ci.length}, the data, no
 *       padding. ts_nsec >= 1e9 is carried into the seconds first, as time.Unix
 *       normalises it.
 *
 * Scope decisions:
 *   - time.Now(). The pcap writer replaces a zero time.Time (ts_sec ==
 *     -62135596800 && ts_nsec == 0) by time.Now(), per packet. Here every zero
 *     time of one call takes the caller's single instant opts->now_sec/now_nsec.
 *   - GPK_CAPW_EBIG. A block of 2^32 bytes or more has no length the format can
 *     carry; the reference would write the wrapped length. Such a packet is
 *     rejected here.
 *   - "capture length %d does not match data length %d" (write.go:118) cannot
 *     occur in a batch, where a packet's data is its caplen bytes. The Python
 *     single-packet path checks it.
 *   - The text of the capture-length error renders the CaptureInfo with Go's
 *     %+v. No reference test pins that text; the Python layer builds it for UTC
 *     times.
 *   - No bufio layer: the reference's NgWriter buffers 4096 bytes and needs
 *     Flush; here the caller gets whole blocks and decides when to write them.
 *
 * A packet in error writes nothing: block_off[j+1] == block_off[j] and
 * status[j] names the check that failed, in the reference's order (interface,
 * then capture length).
 */
#ifndef GPK_CAPWRITE_H
#define GPK_CAPWRITE_H

#include <stddef.h>
#include <stdint.h>

#include "gpk.h"
#include "gpk_capture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_CAPW_PCAP_MICRO 1 /* NewWriter      */
#define GPK_CAPW_PCAP_NANO 2  /* NewWriterNanos */
#define GPK_CAPW_PCAPNG 3     /* NewNgWriter    */

/* status[j] */
#define GPK_CAPW_OK 0
#define GPK_CAPW_ELENGTH (-32)  /* "invalid capture info ...:  capture length > length"  write.go:121, ngwrite.go:368 */
#define GPK_CAPW_EIFACE (-33)   /* "Can't send statistics for non existent interface"    ngwrite.go:302,362; pcapng  */
#define GPK_CAPW_EBIG (-34)     /* the block would be 2^32 bytes or more                                              */
#define GPK_CAPW_EINDEX (-35)   /* order[j] is not a packet of the batch (a caller's error; nothing is read)          */
#define GPK_CAPW_ESECRETS (-36) /* ErrUnknownSecretsType                                 ngwrite_dsb.go:77           */

#define GPK_CAPW_ZERO_TIME_SEC (-62135596800LL) /* time.Time{}.Unix() */

typedef struct gpk_capwriter gpk_capwriter;

/* device >= 0: the writer also owns the device workspace for batches of up to
 * max_packets output packets (< 2^31) on that device; it serves one call at a
 * time. device < 0: a host-only writer (no GPU is touched; gpk_capwrite_batch
 * returns GPK_EINVAL). A pcapng writer starts with no interface. */
int gpk_capwriter_create(gpk_capwriter** out, int format, int device, uint64_t max_packets);
int gpk_capwriter_destroy(gpk_capwriter* w);
/* interfaces added so far (pcapng), or a negative code */
int gpk_capwriter_interfaces(const gpk_capwriter* w);
/* appending to a file that already has n interfaces */
int gpk_capwriter_set_interfaces(gpk_capwriter* w, uint32_t n);

typedef struct gpk_capw_bytes {
  const uint8_t* data;
  uint64_t len;
} gpk_capw_bytes;

/* NgSectionInfo; empty strings are not written */
typedef struct gpk_capw_section {
  gpk_capw_bytes application, comment, hardware, os; /* the order writeSectionHeader writes them in */
} gpk_capw_section;

/* NgInterface, the members AddInterface writes. if_tsresol is always 9. */
typedef struct gpk_capw_interface {
  gpk_capw_bytes name, comment, description, filter, os;
  uint64_t ts_offset; /* written when not 0 */
  uint32_t snap_length;
  uint16_t link_type;
  uint16_t reserved;
} gpk_capw_interface;

/* NgInterfaceStatistics; a zero time.Time (GPK_CAPW_ZERO_TIME_SEC, 0) start or
 * end and a counter of NgNoValue64 (all ones) are not written; a zero
 * last_update is written as 0. */
typedef struct gpk_capw_stats {
  int64_t last_update_sec, start_time_sec, end_time_sec;
  uint32_t last_update_nsec, start_time_nsec, end_time_nsec, reserved;
  uint64_t packets_received, packets_dropped;
} gpk_capw_stats;

/* Writer.WriteFileHeader (write.go:80-96): 24 bytes; a pcap writer only. */
int gpk_capwrite_file_header(const gpk_capwriter* w, uint32_t snaplen, uint32_t link_type, uint8_t* out, uint64_t cap);
/* NgWriter.writeSectionHeader (ngwrite.go:187-234) */
int gpk_capwrite_section_header(const gpk_capwriter* w, const gpk_capw_section* info, uint8_t* out, uint64_t cap);
/* NgWriter.AddInterface (:237-298): *id receives the new interface's number,
 * and the writer counts it, once the block fits cap. The filter option carries
 * its leading 0 byte; the uint8 resolution option is written as 4 bytes. */
int gpk_capwrite_add_interface(gpk_capwriter* w, const gpk_capw_interface* intf, uint8_t* out, uint64_t cap, int* id);
/* NgWriter.WriteInterfaceStats (:301-353): GPK_CAPW_EIFACE unless 0 <= intf < interfaces */
int gpk_capwrite_interface_stats(const gpk_capwriter* w, int64_t intf, const gpk_capw_stats* stats, uint8_t* out,
                                 uint64_t cap);
/* NgWriter.WriteDecryptionSecretsBlock (ngwrite_dsb.go:71-110): GPK_CAPW_ESECRETS
 * for a type that is none of TLS, SSH, WireGuard, Zigbee NWK, Zigbee APS */
int gpk_capwrite_secrets(const gpk_capwriter* w, uint32_t secrets_type, const uint8_t* payload, uint64_t len,
                         uint8_t* out, uint64_t cap);

typedef struct gpk_capwrite_opts {
  int64_t now_sec;   /* pcap formats: the time a zero time.Time is written as */
  uint32_t now_nsec;
  uint32_t group;    /* tests and measurements only: 0 = the library picks the framing kernel's
                        lanes per packet from the batch's mean packet size; 16 or 64 force it */
} gpk_capwrite_opts;

/* Frame packets order[0..m) of a device batch (order NULL: packets 0..m-1;
 * repeats allowed, as in gpk_pack_batch). Device arrays:
 *   ci        [batch->n]  the packets' CaptureInfo (length, iface and time are read)
 *   opt_data, opt_off[m+1]  pcapng: the encoded options of OUTPUT packet j,
 *             end-of-options included, are opt_data[opt_off[j], opt_off[j+1]), a
 *             multiple of 4 bytes; both NULL: no packet has options. Ignored by
 *             the pcap formats.
 *   out       [out_cap], any alignment. Block j is out[block_off[j],
 *             block_off[j+1]). A block that does not end inside out_cap is not
 *             written at all; nothing at or past out + out_cap is touched.
 *   block_off [m+1], status [m]
 *   counts    [4]  blocks written, bytes needed (block_off[m]), packets in
 *             error, overflow (bytes needed > out_cap)
 * opts may be NULL (now = 0, group = 0). Asynchronous on `stream`. Like the
 * project's other byte movers it reads whole aligned 16-byte words around a
 * packet's bytes, so batch->data must be one allocation. */
int gpk_capwrite_batch(gpk_capwriter* w, const gpk_batch* batch, const uint32_t* order, uint64_t m,
                       const gpk_capture_info* ci, const uint8_t* opt_data, const uint64_t* opt_off,
                       const gpk_capwrite_opts* opts, uint8_t* out, uint64_t out_cap, uint64_t* block_off,
                       int32_t* status, uint64_t* counts, void* stream);
/* The same with host pointers, on the calling thread. */
int gpk_capwrite_batch_host(gpk_capwriter* w, const gpk_batch* batch, const uint32_t* order, uint64_t m,
                            const gpk_capture_info* ci, const uint8_t* opt_data, const uint64_t* opt_off,
                            const gpk_capwrite_opts* opts, uint8_t* out, uint64_t out_cap, uint64_t* block_off,
                            int32_t* status, uint64_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* GPK_CAPWRITE_H */
