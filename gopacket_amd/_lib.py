"""ctypes binding of libgpk.so (the C ABI declared in include/gpk.h).

The shared library is built in-tree (gopacket_amd/libgpk.so, see
csrc/Makefile) so the GPU box loads exactly the code in this repository.
There is no fallback: if the library is missing or a call fails, an
exception is raised.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPK_LIB_VARIANT=<name> loads build/libgpk_<name>.so instead: compile-time
# kernel variants built by `make -C gopacket_amd/csrc variant V=<name>
# VDEFS=...` for A/B measurements (tools/ab.sh). Unset in normal use.
_VARIANT = os.environ.get("GPK_LIB_VARIANT")
LIB_PATH = (os.path.join(_HERE, "build", "libgpk_%s.so" % _VARIANT) if _VARIANT
            else os.path.join(_HERE, "libgpk.so"))
SYNTH_PATH = os.path.join(_HERE, "libgpk_synth.so")

# include/gpk.h constants
GPK_OK = 0
GPK_EINVAL, GPK_ENOMEM, GPK_EHIP, GPK_ENODEV, GPK_EUNSUPP = -1, -2, -3, -4, -5
GPK_STOPPED = 1  # a replay or ring pump ended early at gpk_stop (not an error)
OUT_IP4_CSUM, OUT_L4_CSUM, OUT_FLOWS, OUT_ALL = 1, 2, 4, 7
TABLES_AUTO, TABLES_GLOBAL = 0, 1
DEC_NONE, DEC_ETHERNET, DEC_DOT1Q, DEC_IPV4, DEC_IPV6, DEC_IPV6_EXT, DEC_TCP, DEC_UDP, DEC_PAYLOAD, \
    DEC_FRAGMENT = range(10)
ST_ERR_MASK = 0x7F
ST_TRUNCATED = 1 << 7
ST_NLAYERS_SHIFT = 8
ST_NLAYERS_MASK = 0xFFF
ST_IP4_CSUM = 1 << 20
ST_IP4_VALID = 1 << 21
ST_L4_CSUM = 1 << 22
ST_L4_VALID = 1 << 23
ST_L4_UDP = 1 << 24
ST_LINK_FLOW = 1 << 25
ST_NET_FLOW = 1 << 26
ST_NET_IPV6 = 1 << 27
ST_TRANSPORT_FLOW = 1 << 28
LAYOUT_ABSENT = 0xFFFFFFFF
MAX_INLINE_LAYERS = 16

RECORD_DTYPE = np.dtype([("layers", "<u8"), ("status", "<u4"), ("ip4_csum", "<u2"), ("l4_csum", "<u2")])
RECORD8_DTYPE = np.dtype([("layers", "<u4"), ("status", "<u4")])  # gpk_record8 (gpk_decode_batch_narrow)
ST8_NLAYERS_MASK, ST8_WIDE = 0xF, 1 << 12
LAYOUT_DTYPE = np.dtype([("start", "<u4", (8,)), ("end", "<u4", (8,))])
# include/gpk.h gpk_fields (128 B): the scalar layer fields (gpk_extract_fields)
FIELDS_DTYPE = np.dtype({
    "names": ["present", "hbh_opt_map", "eth_type", "eth_length", "eth_dst", "eth_src", "d1q_tci", "d1q_type", "ip4_version",
              "ip4_ihl", "ip4_tos", "ip4_ttl", "ip4_length", "ip4_id", "ip4_flags_frag", "ip4_protocol",
              "ip6_version", "ip4_checksum", "ip6_traffic_class", "ip6_next_header", "ip6_flow_label", "ip6_length",
              "ip6_hop_limit", "tcp_data_offset", "ip4_src", "ip4_dst", "ip6_src", "ip6_dst", "tcp_src_port",
              "tcp_dst_port", "tcp_seq", "tcp_ack", "tcp_flags", "tcp_window", "tcp_checksum", "tcp_urgent",
              "udp_src_port", "udp_dst_port", "udp_length", "udp_checksum", "ip4_start", "tcp_start",
              "ip4_opt_map", "tcp_opt_map"],
    "formats": ["u1", ("u1", (3,)), "<u2", "<u2", ("u1", (6,)), ("u1", (6,)), "<u2", "<u2", "u1", "u1", "u1", "u1", "<u2", "<u2",
                "<u2", "u1", "u1", "<u2", "u1", "u1", "<u4", "<u2", "u1", "u1", ("u1", (4,)), ("u1", (4,)),
                ("u1", (16,)), ("u1", (16,)), "<u2", "<u2", "<u4", "<u4", "<u2", "<u2", "<u2", "<u2", "<u2", "<u2",
                "<u2", "<u2", "u1", "u1", ("u1", (5,)), ("u1", (5,))],
    "offsets": [0, 1, 4, 6, 8, 14, 20, 22, 24, 25, 26, 27, 28, 30, 32, 34, 35, 36, 38, 39, 40, 44, 46, 47, 48, 52, 56, 72,
                88, 90, 92, 96, 100, 102, 104, 106, 108, 110, 112, 114, 116, 117, 118, 123],
    "itemsize": 128})
NAME_FIELDS = 2  # gpk_decode_kernel_name / gpk_decode_occupancy: the fused fields launch
TCP_FLAG_BITS = dict(FIN=1, SYN=2, RST=4, PSH=8, ACK=16, URG=32, ECE=64, CWR=128, NS=256)
# gpk_layout slot -> decoder kind (slot 7: Payload or Fragment)
LAYOUT_SLOTS = (DEC_ETHERNET, DEC_DOT1Q, DEC_IPV4, DEC_IPV6, DEC_IPV6_EXT, DEC_TCP, DEC_UDP, DEC_PAYLOAD)

# exported symbols, in include/gpk.h order
EXPORTS = (
    "gpk_parser_create", "gpk_parser_destroy", "gpk_parser_add_decoder", "gpk_parser_set_options",
    "gpk_parser_set_outputs", "gpk_parser_decoder_for", "gpk_parser_set_ethertype",
    "gpk_parser_set_ipprotocol", "gpk_parser_set_tcp_port", "gpk_parser_set_udp_port", "gpk_ctx_create",
    "gpk_ctx_destroy", "gpk_ctx_set_table_mode", "gpk_stop", "gpk_decode_batch", "gpk_decode_batch_narrow",
    "gpk_decode_batch_narrow_compact", "gpk_wide_collect", "gpk_decode_batch_fields",
    "gpk_extract_fields",
    "gpk_decode_kernel_name", "gpk_decode_occupancy", "gpk_diag_set_buffer", "gpk_decode_batch_host", "gpk_decode_batch_host_fields",
    "gpk_decoded_list",
    "gpk_decoded_list_host", "gpk_host_alloc", "gpk_host_free", "gpk_format_error", "gpk_layer_type_name", "gpk_code_layer_type", "gpk_strerror",
    "gpk_last_hip_error", "gpk_abi_version",
    # include/gpk_capture.h
    "gpk_capreader_create", "gpk_capreader_destroy", "gpk_capreader_index", "gpk_capreader_error",
    "gpk_capreader_link_type", "gpk_capreader_pcap_header", "gpk_capreader_nsections", "gpk_capreader_section_info",
    "gpk_capreader_ninterfaces", "gpk_capreader_interface", "gpk_capreader_interface_str", "gpk_replay_file",
    "gpk_replay_file_range",
    "gpk_capreader_index_all", "gpk_capindex_free",
    "gpk_capreader_section_end_at", "gpk_capreader_nstat_events", "gpk_capreader_stat_event",
    "gpk_capreader_nnames", "gpk_capreader_name", "gpk_capreader_skip_section", "gpk_capreader_set_snaplen",
    "gpk_capreader_keep_options", "gpk_capreader_packet_options",
    # include/gpk_afpacket.h
    "gpk_tp_default_opts", "gpk_tp_check_opts", "gpk_tpacket_new", "gpk_tpacket_attach", "gpk_tpacket_close",
    "gpk_tpacket_ring", "gpk_tpacket_index", "gpk_tpacket_defer", "gpk_tpacket_set_threads", "gpk_tpacket_release_seq", "gpk_tpacket_release",
    "gpk_tpacket_take_new_headers", "gpk_tpacket_geometry", "gpk_tpacket_error", "gpk_tpacket_stats",
    "gpk_tpacket_socket_stats", "gpk_tpacket_set_bpf", "gpk_tpacket_set_fanout", "gpk_tpacket_pump",
    "gpk_tpacket_set_ebpf", "gpk_tpacket_set_promiscuous", "gpk_tpacket_write", "gpk_tpacket_init_socket_stats",
    # include/gpk_flows.h
    "gpk_grouper_create", "gpk_grouper_destroy", "gpk_group_batch", "gpk_pack_batch", "gpk_decode_group_batch",
    "gpk_grouper_hashes",
    # include/gpk_bpf.h
    "gpk_bpf_create", "gpk_bpf_destroy", "gpk_bpf_run", "gpk_bpf_select",
    # include/gpk_defrag.h
    "gpk_defragger_create", "gpk_defragger_destroy", "gpk_defrag_batch", "gpk_defrag_batch_timed",
    # include/gpk_defrag6.h
    "gpk_defragger6_create", "gpk_defragger6_destroy", "gpk_defrag6_batch", "gpk_defrag6_batch_timed",
    # include/gpk_tcpasm.h
    "gpk_tcpasm_create", "gpk_tcpasm_destroy", "gpk_tcpasm_batch", "gpk_tcpasm_batch_timed",
    # include/gpk_capwrite.h
    "gpk_capwriter_create", "gpk_capwriter_destroy", "gpk_capwriter_interfaces", "gpk_capwriter_set_interfaces",
    "gpk_capwrite_file_header", "gpk_capwrite_section_header", "gpk_capwrite_add_interface",
    "gpk_capwrite_interface_stats", "gpk_capwrite_secrets", "gpk_capwrite_batch", "gpk_capwrite_batch_host",
    # include/gpk_serialize.h
    "gpk_serializer_create", "gpk_serializer_destroy", "gpk_serialize_batch", "gpk_serialize_batch_host",
    "gpk_serialize_format_error",
    # include/gpk_tunnel.h
    "gpk_tunneler_create", "gpk_tunneler_destroy", "gpk_tunnel_batch", "gpk_tunnel_batch_host",
    "gpk_tunneler_set_sum_threshold", "gpk_tunnel_format_error",
    # include/gpk_control.h
    "gpk_controller_create", "gpk_controller_destroy", "gpk_control_batch", "gpk_control_batch_host",
    "gpk_controller_set_sum_threshold", "gpk_control_format_error",
    # include/gpk_dns.h
    "gpk_dns_decoder_create", "gpk_dns_decoder_destroy", "gpk_dns_batch", "gpk_dns_batch_host", "gpk_dns_format_error",
    # include/gpk_tls.h
    "gpk_tls_decoder_create", "gpk_tls_decoder_destroy", "gpk_tls_batch", "gpk_tls_batch_host", "gpk_tls_format_error",
    # include/gpk_tls_streams.h
    "gpk_tls_stream_decoder_create", "gpk_tls_stream_decoder_destroy", "gpk_tls_streams", "gpk_tls_streams_host",
    # include/gpk_dns_streams.h
    "gpk_dns_stream_decoder_create", "gpk_dns_stream_decoder_destroy", "gpk_dns_streams", "gpk_dns_streams_host",
    # include/gpk_ndp.h
    "gpk_ndp_decoder_create", "gpk_ndp_decoder_destroy", "gpk_ndp_batch", "gpk_ndp_batch_host", "gpk_ndp_format_error",
    # include/gpk_svc.h
    "gpk_svc_decoder_create", "gpk_svc_decoder_destroy", "gpk_svc_batch", "gpk_svc_batch_host", "gpk_svc_format_error",
)

BPF_INSN_DTYPE = np.dtype([("code", "<u2"), ("jt", "u1"), ("jf", "u1"), ("k", "<u4")])
BPF_MAX_INSNS = 4096

# include/gpk_flows.h constants
GROUP_CONNECTION, GROUP_DEFRAG, GROUP_NET_BUCKET, GROUP_DEFRAG6 = 1, 2, 3, 4
GROUP_NONE, GROUP_USELESS, GROUP_FRAG_TOO_SMALL, GROUP_FRAG_OFFSET, GROUP_FRAG_OVERRUN, GROUP_UNKNOWN = \
    -1, -2, -3, -4, -5, -6


class Groups(ctypes.Structure):
    _fields_ = [("group_of", ctypes.c_void_p), ("perm", ctypes.c_void_p), ("start", ctypes.c_void_p),
                ("first", ctypes.c_void_p), ("counts", ctypes.c_void_p)]

    @classmethod
    def of(cls, groups):
        """From Grouper.group's dict of device tensors."""
        return cls(*[groups[k].data_ptr() for k in ("group_of", "perm", "start", "first", "counts")])


# include/gpk_defrag.h constants
DEFRAG_HELD, DEFRAG_EHOLE, DEFRAG_EINVALID, DEFRAG_EMAXLEN, DEFRAG_EPANIC = -16, -17, -18, -19, -20
DEFRAG_MAX_LIST = 8192


class Datagrams(ctypes.Structure):
    """gpk_datagrams: the outputs of gpk_defrag_batch (device arrays)."""
    _fields_ = [("verdict", ctypes.c_void_p), ("last", ctypes.c_void_p), ("length", ctypes.c_void_p),
                ("offsets", ctypes.c_void_p), ("caplens", ctypes.c_void_p), ("payload_off", ctypes.c_void_p),
                ("pending", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("data", ctypes.c_void_p),
                ("data_cap", ctypes.c_uint64)]


class DefragTime(ctypes.Structure):
    """gpk_defrag_time and gpk_defrag6_time (the same layout): timestamps in,
    DiscardOlderThan(t) after the batch, key times and counts out."""
    _fields_ = [("seen", ctypes.c_void_p), ("discard", ctypes.c_uint32), ("t", ctypes.c_int64),
                ("pending_seen", ctypes.c_void_p), ("counts", ctypes.c_void_p)]


# include/gpk_defrag6.h constants
DEFRAG6_HELD, DEFRAG6_CARRIED = -32, -33
DEFRAG6_MAX_LIST = 8192


class Datagrams6(ctypes.Structure):
    """gpk_datagrams6: the outputs of gpk_defrag6_batch (device arrays)."""
    _fields_ = [("verdict", ctypes.c_void_p), ("last", ctypes.c_void_p), ("head", ctypes.c_void_p),
                ("length", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("caplens", ctypes.c_void_p),
                ("payload_off", ctypes.c_void_p), ("pending", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("data", ctypes.c_void_p), ("data_cap", ctypes.c_uint64)]


# include/gpk_tcpasm.h constants
TCPASM_DIRECT, TCPASM_QUEUED, TCPASM_NOCONN, TCPASM_CARRIED, TCPASM_EBADCARRY, TCPASM_EPANIC = \
    -24, -25, -26, -27, -28, -29
TCPASM_PAGE_BYTES = 1900
TCP_START, TCP_END = 1, 2
TCPASM_CALL_FLUSH, TCPASM_OPEN, TCPASM_NO_CONN = 0x80000000, 0xFFFFFFFF, -2
TCPASM_CARRY_CONN, TCPASM_CARRY_PAGE = 0x80000000, 0x40000000
# gpk_tcp_chunk (40 B): one Reassembly
TCP_CHUNK_DTYPE = np.dtype([("dst", "<u8"), ("skip", "<i8"), ("src", "<u4"), ("src_off", "<u4"), ("len", "<u4"),
                            ("call", "<u4"), ("stream", "<u4"), ("flags", "<u4")])


class TcpasmOpts(ctypes.Structure):
    """gpk_tcpasm_opts"""
    _fields_ = [("max_pages", ctypes.c_uint32), ("flush", ctypes.c_uint32), ("carried", ctypes.c_uint64),
                ("carry_code", ctypes.c_void_p), ("carry_seq", ctypes.c_void_p)]


class TcpasmTime(ctypes.Structure):
    """gpk_tcpasm_time"""
    _fields_ = [("seen", ctypes.c_void_p), ("flush_older", ctypes.c_uint32), ("t", ctypes.c_int64),
                ("conn_last_seen", ctypes.c_void_p), ("counts", ctypes.c_void_p)]


TCPASM_FLUSH_T, TCPASM_FLUSH_T_CLOSE_ALL = 1, 2  # gpk_tcpasm_time.flush_older
TIME_ZERO = -(1 << 63)  # Go's zero time.Time as the reassemblers see it: INT64_MIN


class TcpStreams(ctypes.Structure):
    """gpk_tcp_streams: the outputs of gpk_tcpasm_batch (device arrays)."""
    _fields_ = [("verdict", ctypes.c_void_p), ("stream_of", ctypes.c_void_p), ("chunks", ctypes.c_void_p),
                ("stream_group", ctypes.c_void_p), ("stream_first", ctypes.c_void_p),
                ("stream_closed", ctypes.c_void_p), ("stream_chunk0", ctypes.c_void_p),
                ("stream_data0", ctypes.c_void_p), ("conn_seq", ctypes.c_void_p), ("conn_stream", ctypes.c_void_p),
                ("pend_pkt", ctypes.c_void_p), ("pend_page", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("data", ctypes.c_void_p), ("chunk_cap", ctypes.c_uint64), ("data_cap", ctypes.c_uint64)]


# include/gpk_capwrite.h constants
CAPW_PCAP_MICRO, CAPW_PCAP_NANO, CAPW_PCAPNG = 1, 2, 3
CAPW_OK, CAPW_ELENGTH, CAPW_EIFACE, CAPW_EBIG, CAPW_EINDEX, CAPW_ESECRETS = 0, -32, -33, -34, -35, -36
CAPW_ZERO_TIME_SEC = -62135596800  # time.Time{}.Unix()


class CapwBytes(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class CapwSection(ctypes.Structure):
    _fields_ = [("application", CapwBytes), ("comment", CapwBytes), ("hardware", CapwBytes), ("os", CapwBytes)]


class CapwInterface(ctypes.Structure):
    _fields_ = [("name", CapwBytes), ("comment", CapwBytes), ("description", CapwBytes), ("filter", CapwBytes),
                ("os", CapwBytes), ("ts_offset", ctypes.c_uint64), ("snap_length", ctypes.c_uint32),
                ("link_type", ctypes.c_uint16), ("reserved", ctypes.c_uint16)]


class CapwStats(ctypes.Structure):
    _fields_ = [("last_update_sec", ctypes.c_int64), ("start_time_sec", ctypes.c_int64),
                ("end_time_sec", ctypes.c_int64), ("last_update_nsec", ctypes.c_uint32),
                ("start_time_nsec", ctypes.c_uint32), ("end_time_nsec", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("packets_received", ctypes.c_uint64),
                ("packets_dropped", ctypes.c_uint64)]


class CapwriteOpts(ctypes.Structure):
    """gpk_capwrite_opts"""
    _fields_ = [("now_sec", ctypes.c_int64), ("now_nsec", ctypes.c_uint32), ("group", ctypes.c_uint32)]


# include/gpk_serialize.h constants: status[j] is 0, a reference error (> 0) or a scope code (< 0)
SER_OK = 0
(SER_ERR_ETH_TYPE_LENGTH, SER_ERR_ETH_LENGTH, SER_ERR_IP6_FIT_LEN, SER_ERR_IP6_JUMBO_MISSING,
 SER_ERR_IP6_JUMBO_TLV_LEN, SER_ERR_IP6_JUMBO_SMALL, SER_ERR_IP6_JUMBO_TLV_SHORT, SER_ERR_HBH_MULT8,
 SER_ERR_IP6_FIT, SER_ERR_L4_NO_NETWORK) = range(1, 11)
SER_ENOLAYER, SER_EHBHLONG, SER_EJUMBOADD, SER_EINDEX, SER_ELAYOUT = -40, -41, -42, -43, -44


class SerializeOpts(ctypes.Structure):
    """gpk_serialize_opts"""
    _fields_ = [("fix_lengths", ctypes.c_uint32), ("compute_checksums", ctypes.c_uint32), ("group", ctypes.c_uint32)]


# include/gpk_tunnel.h constants
LT_GRE, LT_VXLAN, LT_GENEVE = 18, 116, 120
TUN_GRE, TUN_VXLAN, TUN_GENEVE, TUN_ALL = 1, 2, 4, 7
TUN_GRE_CSUM = 1
TUN_NONE, TUN_UNKNOWN = -1, -2
(TUN_CLASS_ETHERNET, TUN_CLASS_DOT1Q, TUN_CLASS_IPV4, TUN_CLASS_IPV6, TUN_CLASS_NOINNER,
 TUN_CLASS_FAILED) = range(6)
TUN_NCLASS = 6
(TUN_ERR_VXLAN_SMALL, TUN_ERR_GRE_SMALL, TUN_ERR_GRE_TRUNCATED, TUN_ERR_GENEVE_OPT_SHORT, TUN_ERR_GENEVE_OPT_LEN,
 TUN_ERR_GENEVE_SHORT, TUN_ERR_GENEVE_OPTS_SHORT) = range(70, 77)
TUN_ST_TRUNCATED, TUN_ST_CSUM, TUN_ST_VALID = 1, 2, 4
TUN_VX_I, TUN_VX_G, TUN_VX_D, TUN_VX_A = 1, 2, 4, 8
TUN_GN_O, TUN_GN_C = 1, 2
TUN_SUM_GROUP_BYTES = 8192
# gpk_tunnel (72 B): one decoded tunnel header
TUNNEL_DTYPE = np.dtype([
    ("kind", "u1"), ("err", "u1"), ("status", "u1"), ("bits", "u1"), ("err_a0", "<u4"), ("err_a1", "<u4"),
    ("hdr_off", "<u4"), ("contents_len", "<u4"), ("inner_off", "<u4"), ("inner_len", "<u4"), ("next_type", "<i4"),
    ("vni", "<u4"), ("protocol", "<u2"), ("gbp_id", "<u2"), ("raw0", "u1"), ("raw1", "u1"), ("gre_checksum", "<u2"),
    ("gre_offset", "<u2"), ("gre_correct", "<u2"), ("gre_key", "<u4"), ("gre_seq", "<u4"), ("gre_ack", "<u4"),
    ("count", "<u4"), ("list_off", "<u4"), ("gn_version", "u1"), ("gn_options_length", "u1"), ("reserved", "<u2")])


class Tunnels(ctypes.Structure):
    """gpk_tunnels: the outputs of gpk_tunnel_batch."""
    _fields_ = [("verdict", ctypes.c_void_p), ("class_start", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("in_offsets", ctypes.c_void_p), ("in_caplens", ctypes.c_void_p), ("tunnels", ctypes.c_void_p),
                ("counts", ctypes.c_void_p)]


# include/gpk_control.h constants
LT_ARP, LT_ICMPV4, LT_ICMPV6, LT_ICMPV6_ECHO = 10, 19, 57, 132
CTL_ICMP4, CTL_ICMP6, CTL_ICMP6ECHO, CTL_ARP, CTL_ALL = 1, 2, 4, 8, 15
CTL_CSUM = 1
CTL_NONE, CTL_UNKNOWN = -1, -2
CTL_CLASS_ICMP4, CTL_CLASS_ICMP6, CTL_CLASS_ARP, CTL_CLASS_FAILED = range(4)
CTL_NCLASS = 4
(CTL_ERR_ICMP4_SHORT, CTL_ERR_ICMP6_SHORT, CTL_ERR_ECHO_SHORT, CTL_ERR_ARP_SHORT, CTL_ERR_ARP_EXPECTED) = range(80, 85)
CTL_ST_TRUNCATED, CTL_ST_CSUM, CTL_ST_VALID, CTL_ST_NONET = 1, 2, 4, 8
CTL_SUM_GROUP_BYTES = 8192
# gpk_control (64 B): one candidate's control layers
CONTROL_DTYPE = np.dtype([
    ("kind", "u1"), ("err", "u1"), ("status", "u1"), ("nlayers", "u1"), ("err_a0", "<u4"), ("err_a1", "<u4"),
    ("hdr_off", "<u4"), ("contents_len", "<u4"), ("payload_off", "<u4"), ("payload_len", "<u4"),
    ("unsupported", "<i4"), ("layer_types", "<u2", (3,)), ("typecode", "<u2"), ("checksum", "<u2"),
    ("correct", "<u2"), ("id", "<u2"), ("seq", "<u2"), ("arp_addr_type", "<u2"), ("arp_protocol", "<u2"),
    ("arp_hw_size", "u1"), ("arp_prot_size", "u1"), ("arp_operation", "<u2"), ("next_type", "<i4"),
    ("sum_init", "<u4")])


class Controls(ctypes.Structure):
    """gpk_controls: the outputs of gpk_control_batch."""
    _fields_ = [("verdict", ctypes.c_void_p), ("class_start", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("records", ctypes.c_void_p), ("counts", ctypes.c_void_p)]


# include/gpk_dns.h constants
LT_DNS = 107
DNS_KIND, DNS_ALL = 1, 1
DNS_NONE, DNS_UNKNOWN = -1, -2
DNS_CLASS_OK, DNS_CLASS_FAILED = range(2)
DNS_NCLASS = 2
DNS_ERR_FIRST, DNS_ERR_END = 90, 121  # gpk_dns_err: GPK_DNS_ERR_SHORT .. GPK_DNS_ERR_DNSKEY_SMALL
DNS_ST_TRUNCATED, DNS_ST_DROPPED = 1, 2
DNS_SEC_QUESTION, DNS_SEC_ANSWER, DNS_SEC_AUTHORITY, DNS_SEC_ADDITIONAL = range(4)
# gpk_dns (64 B): one candidate's message
DNS_DTYPE = np.dtype([
    ("kind", "u1"), ("err", "u1"), ("status", "u1"), ("response_code", "u1"), ("err_a0", "<u4"), ("err_a1", "<u4"),
    ("hdr_off", "<u4"), ("len", "<u4"), ("id", "<u2"), ("flags2", "u1"), ("flags3", "u1"), ("qdcount", "<u2"),
    ("ancount", "<u2"), ("nscount", "<u2"), ("arcount", "<u2"), ("nrr", "<u4"), ("reserved", "<u4"), ("rr0", "<u8"),
    ("name0", "<u8"), ("name_bytes", "<u8")])
# gpk_dns_rr (96 B): one question or resource record
DNS_RR_DTYPE = np.dtype([
    ("section", "u1"), ("reserved", "u1"), ("type", "<u2"), ("cls", "<u2"), ("data_length", "<u2"), ("ttl", "<u4"),
    ("data_off", "<u4"), ("name_off", "<u8"), ("name_len", "<u4"), ("count", "<u4"), ("rname_off", "<u8"),
    ("rname_len", "<u4"), ("rname2_len", "<u4"), ("rname2_off", "<u8"), ("v", "<u4", (10,))])


class Dnss(ctypes.Structure):
    """gpk_dnss: the outputs of gpk_dns_batch."""
    _fields_ = [("verdict", ctypes.c_void_p), ("class_start", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("records", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("rrs", ctypes.c_void_p),
                ("names", ctypes.c_void_p), ("rr_cap", ctypes.c_uint64), ("name_cap", ctypes.c_uint64)]


# include/gpk_ndp.h constants
(LT_ICMPV6_ROUTER_SOLICITATION, LT_ICMPV6_ROUTER_ADVERTISEMENT, LT_ICMPV6_NEIGHBOR_SOLICITATION,
 LT_ICMPV6_NEIGHBOR_ADVERTISEMENT, LT_ICMPV6_REDIRECT) = range(124, 129)
LT_MLDV1_REPORT, LT_MLDV1_DONE, LT_MLDV1_QUERY, LT_MLDV2_REPORT, LT_MLDV2_QUERY = range(135, 140)
(NDP_RS, NDP_RA, NDP_NS, NDP_NA, NDP_REDIRECT, NDP_MLD1_QUERY, NDP_MLD1_REPORT, NDP_MLD1_DONE, NDP_MLD2_QUERY,
 NDP_MLD2_REPORT, NDP_ICMP6) = (1 << k for k in range(11))
NDP_MESSAGES, NDP_ALL = 1023, 2047
# layer type -> its bit of the kinds mask
NDP_KIND_OF_TYPE = {
    LT_ICMPV6_ROUTER_SOLICITATION: NDP_RS, LT_ICMPV6_ROUTER_ADVERTISEMENT: NDP_RA,
    LT_ICMPV6_NEIGHBOR_SOLICITATION: NDP_NS, LT_ICMPV6_NEIGHBOR_ADVERTISEMENT: NDP_NA,
    LT_ICMPV6_REDIRECT: NDP_REDIRECT, LT_MLDV1_QUERY: NDP_MLD1_QUERY, LT_MLDV1_REPORT: NDP_MLD1_REPORT,
    LT_MLDV1_DONE: NDP_MLD1_DONE, LT_MLDV2_QUERY: NDP_MLD2_QUERY, LT_MLDV2_REPORT: NDP_MLD2_REPORT}
NDP_NONE, NDP_UNKNOWN = -1, -2
NDP_CLASS_OK, NDP_CLASS_FAILED = range(2)
NDP_NCLASS = 2
NDP_ERR_FIRST, NDP_ERR_END = 140, 155  # gpk_ndp_err: GPK_NDP_ERR_RS_SHORT .. GPK_NDP_ERR_RECORD_AUX
(NDP_ERR_RS_SHORT, NDP_ERR_RA_SHORT, NDP_ERR_NS_SHORT, NDP_ERR_NA_SHORT, NDP_ERR_REDIRECT_SHORT, NDP_ERR_OPT_SHORT,
 NDP_ERR_OPT_ZERO, NDP_ERR_OPT_OVERRUN, NDP_ERR_MLD1_SHORT, NDP_ERR_MLD2_QUERY_SHORT, NDP_ERR_MLD2_QUERY_SOURCES,
 NDP_ERR_MLD2_REPORT_SHORT, NDP_ERR_RECORD_SHORT, NDP_ERR_RECORD_SOURCES, NDP_ERR_RECORD_AUX) = range(140, 155)
NDP_ST_TRUNCATED, NDP_ST_DROPPED = 1, 2
# gpk_ndp (64 B): one candidate's message
NDP_DTYPE = np.dtype([
    ("layer_type", "u1"), ("err", "u1"), ("status", "u1"), ("flags", "u1"), ("err_a0", "<u4"), ("err_a1", "<u4"),
    ("hdr_off", "<u4"), ("len", "<u4"), ("contents_len", "<u4"), ("payload_off", "<u4"), ("payload_len", "<u4"),
    ("v", "<u4", (4,)), ("entry0", "<u8"), ("nentries", "<u4"), ("count", "<u2"), ("s_qrv", "u1"), ("qqic", "u1")])
# gpk_ndp_entry (16 B): one ICMPv6Option or one MLDv2MulticastAddressRecord
NDP_ENTRY_DTYPE = np.dtype([
    ("type", "u1"), ("aux_data_len", "u1"), ("n", "<u2"), ("off", "<u4"), ("ext", "<u4"), ("aux_off", "<u4")])


class Ndps(ctypes.Structure):
    """gpk_ndps: the outputs of gpk_ndp_batch."""
    _fields_ = [("verdict", ctypes.c_void_p), ("class_start", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("records", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("entries", ctypes.c_void_p),
                ("entry_cap", ctypes.c_uint64)]


# include/gpk_svc.h constants
LT_NTP, LT_DHCPV4, LT_DHCPV6 = 117, 118, 134
SVC_DHCP4, SVC_DHCP6, SVC_NTP = 1, 2, 4
SVC_ALL = 7
SVC_KIND_OF_TYPE = {LT_DHCPV4: SVC_DHCP4, LT_DHCPV6: SVC_DHCP6, LT_NTP: SVC_NTP}  # layer type -> its bit of the kinds mask
SVC_NONE, SVC_UNKNOWN = -1, -2
SVC_CLASS_OK, SVC_CLASS_FAILED = range(2)
SVC_NCLASS = 2
SVC_ERR_FIRST, SVC_ERR_END = 160, 170  # gpk_svc_err: GPK_SVC_ERR_DHCP4_SHORT .. GPK_SVC_ERR_NTP_SHORT
(SVC_ERR_DHCP4_SHORT, SVC_ERR_DHCP4_HLEN, SVC_ERR_DHCP4_MAGIC, SVC_ERR_DHCP4_OPT_SHORT, SVC_ERR_DHCP4_OPT_MALFORMED,
 SVC_ERR_DHCP6_SHORT, SVC_ERR_DHCP6_RELAY_SHORT, SVC_ERR_DHCP6_OPT_SHORT, SVC_ERR_DHCP6_OPT_LENGTH,
 SVC_ERR_NTP_SHORT) = range(160, 170)
SVC_ST_TRUNCATED, SVC_ST_DROPPED = 1, 2
# gpk_svc (64 B): one candidate's message
SVC_DTYPE = np.dtype([
    ("layer_type", "u1"), ("err", "u1"), ("status", "u1"), ("reserved", "u1"), ("err_a0", "<u4"), ("err_a1", "<u4"),
    ("hdr_off", "<u4"), ("len", "<u4"), ("contents_len", "<u4"), ("entry0", "<u8"), ("nentries", "<u4"),
    ("b", "u1", (4,)), ("v", "<u4", (6,))])
# gpk_svc_entry (8 B): one DHCPOption or one DHCPv6Option
SVC_ENTRY_DTYPE = np.dtype([("code", "<u2"), ("length", "<u2"), ("off", "<u4")])


class Svcs(ctypes.Structure):
    """gpk_svcs: the outputs of gpk_svc_batch."""
    _fields_ = [("verdict", ctypes.c_void_p), ("class_start", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("records", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("entries", ctypes.c_void_p),
                ("entry_cap", ctypes.c_uint64)]


# include/gpk_tls.h constants
LT_TLS = 140
TLS_KIND, TLS_ALL = 1, 1
TLS_NONE, TLS_UNKNOWN = -1, -2
TLS_CLASS_OK, TLS_CLASS_FAILED = range(2)
TLS_NCLASS = 2
TLS_ERR_FIRST, TLS_ERR_END = 121, 133  # gpk_tls_err: GPK_TLS_ERR_RECORD_SHORT .. GPK_TLS_ERR_HELLO_EXTENSIONS
TLS_ST_TRUNCATED, TLS_ST_DROPPED = 1, 2
TLS_HS_NONE, TLS_HS_ENCRYPTED, TLS_HS_CLIENT_HELLO, TLS_HS_CLIENT_KEY = range(4)
TLS_NO_HELLO = 0xFFFFFFFF
ERR_PANIC_SLICE_B = 4  # gpk.h: the one panic form of the TLS path
# gpk_tls (80 B): one candidate's message
TLS_DTYPE = np.dtype([
    ("err", "u1"), ("status", "u1"), ("reserved", "<u2"), ("err_a0", "<u4"), ("err_a1", "<u4"), ("hdr_off", "<u4"),
    ("len", "<u4"), ("nrec", "<u4"), ("nccs", "<u4"), ("nalert", "<u4"), ("nhandshake", "<u4"), ("nappdata", "<u4"),
    ("nhello", "<u4"), ("reserved2", "<u4"), ("sni_bytes", "<u8"), ("rec0", "<u8"), ("hello0", "<u8"), ("sni0", "<u8")])
# gpk_tls_rec (16 B): one TLS record
TLS_REC_DTYPE = np.dtype([
    ("content_type", "u1"), ("hs", "u1"), ("v0", "u1"), ("v1", "u1"), ("version", "<u2"), ("length", "<u2"),
    ("body_off", "<u4"), ("hello", "<u4")])
# gpk_tls_hello (64 B): one decoded ClientHello
TLS_HELLO_DTYPE = np.dtype([
    ("handshake_type", "u1"), ("session_id_length", "u1"), ("compression_methods_length", "u1"), ("has_sni", "u1"),
    ("length", "<u4"), ("protocol_version", "<u2"), ("cipher_suits_length", "<u2"), ("extensions_length", "<u2"),
    ("reserved", "<u2"), ("packet", "<u4"), ("random_off", "<u4"), ("session_id_off", "<u4"),
    ("cipher_suits_off", "<u4"), ("compression_methods_off", "<u4"), ("extensions_off", "<u4"), ("sni_off", "<u4"),
    ("sni_len", "<u4"), ("sni_pos", "<u8"), ("reserved2", "<u8")])


class Tlss(ctypes.Structure):
    """gpk_tlss: the outputs of gpk_tls_batch."""
    _fields_ = [("verdict", ctypes.c_void_p), ("class_start", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("records", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("recs", ctypes.c_void_p),
                ("hellos", ctypes.c_void_p), ("snis", ctypes.c_void_p), ("rec_cap", ctypes.c_uint64),
                ("hello_cap", ctypes.c_uint64), ("sni_cap", ctypes.c_uint64)]


# include/gpk_tls_streams.h constants
TLSS_NEW, TLSS_SYNCED, TLSS_NONE, TLSS_NOSTART, TLSS_NOT_TLS, TLSS_LOST, TLSS_CLOSED = range(7)
TLSS_NSTATE = 7
TLSS_ST_DROPPED, TLSS_ST_TOOBIG, TLSS_ST_BADTAIL = 1, 2, 4
TLSS_FRAME_UNSTARTED = 1
TLSS_MAX_TAIL = 65539
# gpk_tls_stream (64 B): one stream of a call
TLS_STREAM_DTYPE = np.dtype([
    ("state", "u1"), ("status", "u1"), ("reserved", "<u2"), ("tail_in", "<u4"), ("consumed", "<u4"),
    ("tail_len", "<u4"), ("tail_off", "<u8"), ("nrec", "<u4"), ("nfailed", "<u4"), ("nhello", "<u4"),
    ("sni_bytes", "<u4"), ("rec0", "<u8"), ("hello0", "<u8"), ("sni0", "<u8")])
# gpk_tls_stream_rec (32 B): one record of a stream
TLS_STREAM_REC_DTYPE = np.dtype([
    ("rec", TLS_REC_DTYPE), ("err", "u1"), ("status", "u1"), ("reserved", "<u2"), ("err_a0", "<u4"), ("err_a1", "<u4"),
    ("stream", "<u4")])


class TlsStreamIn(ctypes.Structure):
    """gpk_tls_stream_in: what the streams carry into a gpk_tls_streams call."""
    _fields_ = [("state", ctypes.c_void_p), ("tail_off", ctypes.c_void_p), ("tail_len", ctypes.c_void_p),
                ("tails", ctypes.c_void_p), ("n", ctypes.c_uint64), ("tail_bytes", ctypes.c_uint64),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class TlsStreamOut(ctypes.Structure):
    """gpk_tls_stream_out: the outputs of gpk_tls_streams."""
    _fields_ = [("streams", ctypes.c_void_p), ("recs", ctypes.c_void_p), ("hellos", ctypes.c_void_p),
                ("snis", ctypes.c_void_p), ("tails", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("rec_cap", ctypes.c_uint64), ("hello_cap", ctypes.c_uint64), ("sni_cap", ctypes.c_uint64),
                ("tail_cap", ctypes.c_uint64)]


# include/gpk_dns_streams.h constants
DNSS_NEW, DNSS_SYNCED, DNSS_NONE, DNSS_NOSTART, DNSS_LOST, DNSS_CLOSED = range(6)
DNSS_NSTATE = 6
DNSS_ST_DROPPED, DNSS_ST_TOOBIG, DNSS_ST_BADTAIL = 1, 2, 4
DNSS_MSG_PARTIAL, DNSS_MSG_SKIPPED, DNSS_MSG_DROPPED = 1, 2, 4
DNSS_FRAME_UNSTARTED = 1
DNSS_MAX_TAIL = 65536
# gpk_dns_stream (64 B): one stream of a call
DNS_STREAM_DTYPE = np.dtype([
    ("state", "u1"), ("status", "u1"), ("reserved", "<u2"), ("tail_in", "<u4"), ("consumed", "<u4"),
    ("tail_len", "<u4"), ("tail_off", "<u8"), ("nmsg", "<u4"), ("nfailed", "<u4"), ("msg0", "<u8"),
    ("reserved2", "<u8", (3,))])
# gpk_dns_stream_msg (80 B): one message of a stream
DNS_STREAM_MSG_DTYPE = np.dtype([
    ("msg", DNS_DTYPE), ("stream", "<u4"), ("status", "u1"), ("reserved", "u1", (3,)), ("present", "<u4"),
    ("reserved2", "<u4")])


class DnsStreamIn(ctypes.Structure):
    """gpk_dns_stream_in: what the streams carry into a gpk_dns_streams call."""
    _fields_ = [("state", ctypes.c_void_p), ("tail_off", ctypes.c_void_p), ("tail_len", ctypes.c_void_p),
                ("tails", ctypes.c_void_p), ("n", ctypes.c_uint64), ("tail_bytes", ctypes.c_uint64),
                ("flags", ctypes.c_uint32), ("max_msg_len", ctypes.c_uint32)]


class DnsStreamOut(ctypes.Structure):
    """gpk_dns_stream_out: the outputs of gpk_dns_streams."""
    _fields_ = [("streams", ctypes.c_void_p), ("msgs", ctypes.c_void_p), ("rrs", ctypes.c_void_p),
                ("names", ctypes.c_void_p), ("tails", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("msg_cap", ctypes.c_uint64), ("rr_cap", ctypes.c_uint64), ("name_cap", ctypes.c_uint64),
                ("tail_cap", ctypes.c_uint64)]


# include/gpk_afpacket.h constants
TPACKET_V1, TPACKET_V2, TPACKET_V3, TPACKET_HIGHEST = 0, 1, 2, -1
TP_WAIT, TP_FULL, TP_ERROR = 0, 1, 2
TPINFO_DTYPE = np.dtype([("ts_sec", "<i8"), ("ts_nsec", "<u4"), ("length", "<u4"), ("iface", "<i4"),
                         ("vlan", "<i4")])


class TpOpts(ctypes.Structure):
    _fields_ = [("version", ctypes.c_int32), ("socktype", ctypes.c_int32), ("frame_size", ctypes.c_int32),
                ("block_size", ctypes.c_int32), ("num_blocks", ctypes.c_int32), ("frames_per_block", ctypes.c_int32),
                ("add_vlan_header", ctypes.c_int32), ("vnet_hdr_size", ctypes.c_int32),
                ("block_timeout_ns", ctypes.c_int64), ("poll_timeout_ns", ctypes.c_int64),
                ("protocol", ctypes.c_uint16), ("_pad", ctypes.c_uint16 * 3), ("iface", ctypes.c_char * 64)]


# gpk_tp_pump_fields_cb(user, first_packet, n, const gpk_fields*)
PUMP_FIELDS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p)


# gpk_tp_pump_packets_cb(user, first_packet, n, const uint8_t* const* data, const uint32_t* caplens)
PUMP_PACKETS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                   ctypes.c_void_p)


class PumpOpts(ctypes.Structure):
    _fields_ = [("batch_pkts", ctypes.c_uint64), ("max_packets", ctypes.c_uint64), ("wait", ctypes.c_int),
                ("inflight", ctypes.c_int), ("fields_cb", PUMP_FIELDS_CB), ("packets_cb", PUMP_PACKETS_CB)]


class PumpStats(ctypes.Structure):
    _fields_ = [("packets", ctypes.c_uint64), ("packet_bytes", ctypes.c_uint64), ("batches", ctypes.c_uint64),
                ("ring_bytes_copied", ctypes.c_uint64), ("waits", ctypes.c_uint64), ("wall_s", ctypes.c_double),
                ("index_s", ctypes.c_double), ("gpu_s", ctypes.c_double), ("kernel_s", ctypes.c_double),
                ("status", ctypes.c_int), ("error", ctypes.c_char * 160), ("kernel", ctypes.c_char * 96)]


PUMP_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)

# include/gpk_capture.h constants
CAP_PCAP, CAP_PCAPNG = 1, 2
NG_WANT_MIXED_LINKTYPE, NG_ERROR_ON_MISMATCHING_LINKTYPE, NG_SKIP_UNKNOWN_VERSION = 1, 2, 4
CAP_MORE, CAP_FULL, CAP_END = 0, 1, 2
CAPINFO_DTYPE = np.dtype([("ts_sec", "<i8"), ("ts_nsec", "<u4"), ("length", "<u4"), ("iface", "<i4"),
                          ("link_type", "<i4")])


class CapIndex(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("offsets", ctypes.c_void_p), ("caplens", ctypes.c_void_p),
                ("ci", ctypes.c_void_p)]


class NgInterface(ctypes.Structure):
    _fields_ = [("link_type", ctypes.c_uint16), ("ts_resolution", ctypes.c_uint8),
                ("has_statistics", ctypes.c_uint8), ("snap_length", ctypes.c_uint32), ("ts_offset", ctypes.c_uint64),
                ("last_update_sec", ctypes.c_int64), ("start_time_sec", ctypes.c_int64),
                ("end_time_sec", ctypes.c_int64), ("last_update_nsec", ctypes.c_uint32),
                ("start_time_nsec", ctypes.c_uint32), ("end_time_nsec", ctypes.c_uint32), ("_pad", ctypes.c_uint32),
                ("packets_received", ctypes.c_uint64), ("packets_dropped", ctypes.c_uint64)]


# gpk_replay_fields_cb(user, first_packet, n, const gpk_fields*)
REPLAY_FIELDS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p)
# gpk_replay_packets_cb(user, first_packet, n, base, bytes, offsets, caplens)
REPLAY_PACKETS_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p)


class ReplayOpts(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int), ("ng_flags", ctypes.c_uint32), ("slot_bytes", ctypes.c_uint64),
                ("slots", ctypes.c_int), ("batch_pkts", ctypes.c_uint64), ("read_threads", ctypes.c_int),
                ("fields_cb", REPLAY_FIELDS_CB), ("packets_cb", REPLAY_PACKETS_CB)]


class ReplayStats(ctypes.Structure):
    _fields_ = [("packets", ctypes.c_uint64), ("packet_bytes", ctypes.c_uint64), ("file_bytes", ctypes.c_uint64),
                ("stream_bytes", ctypes.c_uint64), ("batches", ctypes.c_uint64), ("slots", ctypes.c_uint64),
                ("wall_s", ctypes.c_double), ("read_s", ctypes.c_double), ("index_s", ctypes.c_double),
                ("gpu_s", ctypes.c_double), ("kernel_s", ctypes.c_double), ("deliver_s", ctypes.c_double),
                ("reader_status", ctypes.c_int), ("error", ctypes.c_char * 160), ("kernel", ctypes.c_char * 96),
                ("device_walk_packets", ctypes.c_uint64), ("alloc_wait_s", ctypes.c_double)]


class ReplayRange(ctypes.Structure):
    _fields_ = [("begin", ctypes.c_uint64), ("end", ctypes.c_uint64), ("header_end", ctypes.c_uint64),
                ("sync_begin", ctypes.c_uint64), ("sync_end", ctypes.c_uint64), ("clean", ctypes.c_int),
                ("state_changed", ctypes.c_int)]


REPLAY_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)


class GpkError(RuntimeError):
    """A negative status from the C ABI."""


class Batch(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("caplens", ctypes.c_void_p),
                ("n", ctypes.c_uint64), ("data_bytes", ctypes.c_uint64)]

    @classmethod
    def of(cls, data, offsets, caplens):
        """From the three device tensors of a batch."""
        return cls(data.data_ptr(), offsets.data_ptr(), caplens.data_ptr(), offsets.numel(), data.numel())


class Results(ctypes.Structure):
    _fields_ = [("records", ctypes.c_void_p), ("err_args", ctypes.c_void_p), ("flows", ctypes.c_void_p),
                ("layouts", ctypes.c_void_p)]


class Results8(ctypes.Structure):
    _fields_ = [("records", ctypes.c_void_p), ("wide", ctypes.c_void_p), ("err_args", ctypes.c_void_p),
                ("flows", ctypes.c_void_p)]


WIDE_COUNT_STRIDE = 32  # GPK_WIDE_COUNT_STRIDE: u32 words between two shards' counters


class WideList(ctypes.Structure):
    """gpk_wide_list: the sharded list of widened records (gpk_decode_batch_narrow_compact)."""
    _fields_ = [("index", ctypes.c_void_p), ("records", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("nshards", ctypes.c_uint32), ("shard_cap", ctypes.c_uint32)]


_lib = None


def _share_hip_runtime():
    """One HIP runtime per process. PyTorch-ROCm ships its own libamdhip64
    (SONAME libamdhip64.so.7, NEEDED as "libamdhip64.so" by libtorch_hip), so
    if libgpk.so were loaded first the process would end up with two HIP/HSA
    runtimes and the second one finds no device. Importing torch first makes
    libgpk's libamdhip64.so.7 resolve to torch's already-loaded copy."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("gopacket_amd: %s is not built (run __graft_entry__.build() or make -C "
                          "gopacket_amd/csrc)" % LIB_PATH)
    _share_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, u32, u64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    P = ctypes.POINTER
    sig = {
        "gpk_parser_create": ([P(vp), i64], c_int),
        "gpk_parser_destroy": ([vp], c_int),
        "gpk_parser_add_decoder": ([vp, c_int], c_int),
        "gpk_parser_set_options": ([vp, c_int, c_int], c_int),
        "gpk_parser_set_outputs": ([vp, u32], c_int),
        "gpk_parser_decoder_for": ([vp, i64], c_int),
        "gpk_parser_set_ethertype": ([vp, u32, ctypes.c_int32], c_int),
        "gpk_parser_set_ipprotocol": ([vp, u32, ctypes.c_int32], c_int),
        "gpk_parser_set_tcp_port": ([vp, u32, ctypes.c_int32], c_int),
        "gpk_parser_set_udp_port": ([vp, u32, ctypes.c_int32], c_int),
        "gpk_ctx_create": ([P(vp), c_int], c_int),
        "gpk_ctx_destroy": ([vp], c_int),
        "gpk_ctx_set_table_mode": ([vp, c_int], c_int),
        "gpk_stop": ([vp], c_int),
        "gpk_decode_batch": ([vp, vp, P(Batch), P(Results), vp], c_int),
        "gpk_decode_batch_narrow": ([vp, vp, P(Batch), P(Results8), vp], c_int),
        "gpk_decode_batch_narrow_compact": ([vp, vp, P(Batch), P(Results8), P(WideList), vp], c_int),
        "gpk_wide_collect": ([P(WideList), vp, vp, P(u64), P(u64)], c_int),
        "gpk_decode_batch_host": ([vp, vp, P(Batch), P(Results)], c_int),
        "gpk_decode_batch_host_fields": ([vp, vp, P(Batch), P(Results), vp], c_int),
        "gpk_extract_fields": ([P(Batch), vp, vp, vp], c_int),
        "gpk_decode_batch_fields": ([vp, vp, P(Batch), P(Results), vp, vp], c_int),
        "gpk_decode_kernel_name": ([vp, vp, P(Batch), c_int, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_decode_occupancy": ([vp, vp, P(Batch), c_int, P(c_int)], c_int),
        "gpk_diag_set_buffer": ([vp], c_int),
        "gpk_decoded_list": ([vp, vp, P(Batch), u64, P(i64), u32, P(u32)], c_int),
        "gpk_decoded_list_host": ([vp, vp, ctypes.c_char_p, u32, P(i64), u32, P(u32)], c_int),
        "gpk_host_alloc": ([P(vp), ctypes.c_size_t], c_int),
        "gpk_host_free": ([vp], c_int),
        "gpk_format_error": ([ctypes.c_uint, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_layer_type_name": ([i64, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_code_layer_type": ([ctypes.c_uint], i64),
        "gpk_strerror": ([c_int], ctypes.c_char_p),
        "gpk_last_hip_error": ([], ctypes.c_char_p),
        "gpk_abi_version": ([], c_int),
        "gpk_capreader_create": ([P(vp), c_int, u32], c_int),
        "gpk_capreader_destroy": ([vp], c_int),
        "gpk_capreader_index": ([vp, vp, u64, c_int, vp, vp, vp, u64, P(u64), P(u64)], c_int),
        "gpk_capreader_error": ([vp, ctypes.c_char_p, ctypes.c_size_t, P(c_int), P(c_int)], c_int),
        "gpk_capreader_link_type": ([vp], c_int),
        "gpk_capreader_pcap_header": ([vp, P(u32), P(ctypes.c_uint16), P(ctypes.c_uint16), P(c_int)], c_int),
        "gpk_capreader_nsections": ([vp], c_int),
        "gpk_capreader_section_info": ([vp, c_int, c_int, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_capreader_ninterfaces": ([vp, c_int], c_int),
        "gpk_capreader_interface": ([vp, c_int, c_int, P(NgInterface)], c_int),
        "gpk_capreader_interface_str": ([vp, c_int, c_int, c_int, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_capreader_section_end_at": ([vp, c_int, P(ctypes.c_uint64), P(ctypes.c_uint64)], c_int),
        "gpk_capreader_nstat_events": ([vp], c_int),
        "gpk_capreader_stat_event": ([vp, c_int, P(ctypes.c_uint64), P(ctypes.c_uint64), P(c_int), P(NgInterface),
                                      ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_capreader_nnames": ([vp], c_int),
        "gpk_capreader_name": ([vp, c_int, P(c_int), vp, P(c_int), P(c_int), ctypes.c_char_p, ctypes.c_size_t],
                               c_int),
        "gpk_capreader_skip_section": ([vp], c_int),
        "gpk_capreader_set_snaplen": ([vp, ctypes.c_uint32], c_int),
        "gpk_capreader_keep_options": ([vp, c_int], c_int),
        "gpk_capreader_packet_options": ([vp, ctypes.c_uint64, P(vp), P(ctypes.c_uint64)], c_int),
        "gpk_replay_file": ([vp, vp, ctypes.c_char_p, P(ReplayOpts), REPLAY_CB, vp, P(ReplayStats)], c_int),
        "gpk_replay_file_range": ([vp, vp, ctypes.c_char_p, P(ReplayRange), P(ReplayOpts), REPLAY_CB, vp,
                                   P(ReplayStats)], c_int),
        "gpk_capreader_index_all": ([vp, vp, u64, c_int, c_int, P(CapIndex), P(u64)], c_int),
        "gpk_capindex_free": ([P(CapIndex)], c_int),
        "gpk_tp_default_opts": ([P(TpOpts)], None),
        "gpk_tp_check_opts": ([P(TpOpts), ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_tpacket_new": ([P(vp), P(TpOpts), ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_tpacket_attach": ([P(vp), vp, u64, c_int, P(TpOpts)], c_int),
        "gpk_tpacket_close": ([vp], c_int),
        "gpk_tpacket_ring": ([vp, P(vp), P(u64), P(c_int), P(c_int)], c_int),
        "gpk_tpacket_index": ([vp, c_int, vp, vp, vp, u64, P(u64), vp, u64, P(u64)], c_int),
        "gpk_tpacket_defer": ([vp, c_int], c_int),
        "gpk_tpacket_set_threads": ([vp, c_int], c_int),
        "gpk_tpacket_release_seq": ([vp, P(u64)], c_int),
        "gpk_tpacket_release": ([vp, u64], c_int),
        "gpk_tpacket_take_new_headers": ([vp, P(u64), P(u64)], c_int),
        "gpk_tpacket_geometry": ([vp, P(u64), P(u64)], c_int),
        "gpk_tpacket_error": ([vp, ctypes.c_char_p, ctypes.c_size_t, P(c_int)], c_int),
        "gpk_tpacket_stats": ([vp, P(i64), P(i64)], c_int),
        "gpk_tpacket_socket_stats": ([vp, P(u32), P(u32), P(u32)], c_int),
        "gpk_tpacket_set_bpf": ([vp, vp, u32], c_int),
        "gpk_tpacket_set_fanout": ([vp, c_int, ctypes.c_uint16], c_int),
        "gpk_tpacket_set_ebpf": ([vp, ctypes.c_int32], c_int),
        "gpk_tpacket_set_promiscuous": ([vp, c_int], c_int),
        "gpk_tpacket_write": ([vp, vp, ctypes.c_uint64], c_int),
        "gpk_tpacket_init_socket_stats": ([vp], c_int),
        "gpk_tpacket_pump": ([vp, vp, vp, P(PumpOpts), PUMP_CB, vp, P(PumpStats)], c_int),
        "gpk_grouper_create": ([P(vp), c_int, u64], c_int),
        "gpk_grouper_destroy": ([vp], c_int),
        "gpk_grouper_hashes": ([vp, u64, vp], c_int),
        "gpk_group_batch": ([vp, P(Batch), P(Results), c_int, u32, P(Groups), vp], c_int),
        "gpk_pack_batch": ([P(Batch), vp, u64, vp, vp, vp, vp], c_int),
        "gpk_decode_group_batch": ([vp, vp, P(Batch), P(Results), vp, c_int, P(Groups), vp], c_int),
        "gpk_defragger_create": ([P(vp), c_int, u64], c_int),
        "gpk_defragger_destroy": ([vp], c_int),
        "gpk_defrag_batch": ([vp, P(Batch), P(Results), P(Groups), P(Datagrams), vp], c_int),
        "gpk_defrag_batch_timed": ([vp, P(Batch), P(Results), P(Groups), P(Datagrams), P(DefragTime), vp], c_int),
        "gpk_defragger6_create": ([P(vp), c_int, u64], c_int),
        "gpk_defragger6_destroy": ([vp], c_int),
        "gpk_defrag6_batch": ([vp, P(Batch), P(Results), P(Groups), u64, P(Datagrams6), vp], c_int),
        "gpk_defrag6_batch_timed": ([vp, P(Batch), P(Results), P(Groups), u64, P(Datagrams6), P(DefragTime), vp],
                                    c_int),
        "gpk_tcpasm_create": ([P(vp), c_int, u64], c_int),
        "gpk_tcpasm_destroy": ([vp], c_int),
        "gpk_tcpasm_batch": ([vp, P(Batch), P(Results), P(Groups), P(TcpasmOpts), P(TcpStreams), vp], c_int),
        "gpk_tcpasm_batch_timed": ([vp, P(Batch), P(Results), P(Groups), P(TcpasmOpts), P(TcpStreams), P(TcpasmTime),
                                    vp], c_int),
        "gpk_capwriter_create": ([P(vp), c_int, c_int, u64], c_int),
        "gpk_capwriter_destroy": ([vp], c_int),
        "gpk_capwriter_interfaces": ([vp], c_int),
        "gpk_capwriter_set_interfaces": ([vp, u32], c_int),
        "gpk_capwrite_file_header": ([vp, u32, u32, vp, u64], c_int),
        "gpk_capwrite_section_header": ([vp, P(CapwSection), vp, u64], c_int),
        "gpk_capwrite_add_interface": ([vp, P(CapwInterface), vp, u64, P(c_int)], c_int),
        "gpk_capwrite_interface_stats": ([vp, i64, P(CapwStats), vp, u64], c_int),
        "gpk_capwrite_secrets": ([vp, u32, vp, u64, vp, u64], c_int),
        "gpk_capwrite_batch": ([vp, P(Batch), vp, u64, vp, vp, vp, P(CapwriteOpts), vp, u64, vp, vp, vp, vp], c_int),
        "gpk_capwrite_batch_host": ([vp, P(Batch), vp, u64, vp, vp, vp, P(CapwriteOpts), vp, u64, vp, vp, vp],
                                    c_int),
        "gpk_serializer_create": ([P(vp), c_int, u64], c_int),
        "gpk_serializer_destroy": ([vp], c_int),
        "gpk_serialize_batch": ([vp, P(Batch), vp, vp, vp, u64, P(SerializeOpts), vp, u64, vp, vp, vp, vp, vp, vp],
                                c_int),
        "gpk_serialize_batch_host": ([vp, P(Batch), vp, vp, vp, u64, P(SerializeOpts), vp, u64, vp, vp, vp, vp, vp],
                                     c_int),
        "gpk_serialize_format_error": ([c_int, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_tunneler_create": ([P(vp), c_int, u64], c_int),
        "gpk_tunneler_destroy": ([vp], c_int),
        "gpk_tunnel_batch": ([vp, vp, vp, P(Batch), P(Results), u32, u32, P(Tunnels), vp], c_int),
        "gpk_tunnel_batch_host": ([vp, P(Batch), P(Results), u32, u32, P(Tunnels)], c_int),
        "gpk_tunneler_set_sum_threshold": ([vp, u32], c_int),
        "gpk_tunnel_format_error": ([ctypes.c_uint, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_controller_create": ([P(vp), c_int, u64], c_int),
        "gpk_controller_destroy": ([vp], c_int),
        "gpk_control_batch": ([vp, vp, vp, P(Batch), P(Results), u32, u32, P(Controls), vp], c_int),
        "gpk_control_batch_host": ([vp, P(Batch), P(Results), u32, u32, P(Controls)], c_int),
        "gpk_controller_set_sum_threshold": ([vp, u32], c_int),
        "gpk_control_format_error": ([ctypes.c_uint, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_dns_decoder_create": ([P(vp), c_int, u64], c_int),
        "gpk_dns_decoder_destroy": ([vp], c_int),
        "gpk_dns_batch": ([vp, vp, vp, P(Batch), P(Results), P(Dnss), vp], c_int),
        "gpk_dns_batch_host": ([vp, P(Batch), P(Results), P(Dnss)], c_int),
        "gpk_dns_format_error": ([ctypes.c_uint, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_tls_decoder_create": ([P(vp), c_int, u64], c_int),
        "gpk_tls_decoder_destroy": ([vp], c_int),
        "gpk_tls_batch": ([vp, vp, vp, P(Batch), P(Results), P(Tlss), vp], c_int),
        "gpk_tls_batch_host": ([vp, P(Batch), P(Results), P(Tlss)], c_int),
        "gpk_tls_format_error": ([ctypes.c_uint, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_tls_stream_decoder_create": ([P(vp), c_int, u64], c_int),
        "gpk_tls_stream_decoder_destroy": ([vp], c_int),
        "gpk_tls_streams": ([vp, vp, vp, P(Batch), P(Results), P(TcpStreams), P(TlsStreamIn), P(TlsStreamOut), vp],
                            c_int),
        "gpk_tls_streams_host": ([vp, P(Batch), P(Results), P(TcpStreams), P(TlsStreamIn), P(TlsStreamOut)], c_int),
        "gpk_dns_stream_decoder_create": ([P(vp), c_int, u64, u64], c_int),
        "gpk_dns_stream_decoder_destroy": ([vp], c_int),
        "gpk_dns_streams": ([vp, vp, vp, P(Batch), P(Results), P(TcpStreams), P(DnsStreamIn), P(DnsStreamOut), vp],
                            c_int),
        "gpk_dns_streams_host": ([vp, P(Batch), P(Results), P(TcpStreams), P(DnsStreamIn), P(DnsStreamOut)], c_int),
        "gpk_ndp_decoder_create": ([P(vp), c_int, u64], c_int),
        "gpk_ndp_decoder_destroy": ([vp], c_int),
        "gpk_ndp_batch": ([vp, vp, vp, P(Batch), P(Results), u32, P(Ndps), vp], c_int),
        "gpk_ndp_batch_host": ([vp, P(Batch), P(Results), u32, P(Ndps)], c_int),
        "gpk_ndp_format_error": ([ctypes.c_uint, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_svc_decoder_create": ([P(vp), c_int, u64], c_int),
        "gpk_svc_decoder_destroy": ([vp], c_int),
        "gpk_svc_batch": ([vp, vp, vp, P(Batch), P(Results), u32, P(Svcs), vp], c_int),
        "gpk_svc_batch_host": ([vp, P(Batch), P(Results), u32, P(Svcs)], c_int),
        "gpk_svc_format_error": ([ctypes.c_uint, u32, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_bpf_create": ([P(vp), vp, u32, ctypes.c_char_p, ctypes.c_size_t], c_int),
        "gpk_bpf_destroy": ([vp], c_int),
        "gpk_bpf_run": ([vp, P(Batch), vp, vp, vp], c_int),
        "gpk_bpf_select": ([vp, P(Batch), vp, vp, vp, vp, vp, vp], c_int),
    }
    for name, (args, res) in sig.items():
        if _VARIANT and not hasattr(L, name):
            continue  # a kernel variant library: the decode ABI only (gpk_kernels.hip + gpk_host.cpp)
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def check(rc):
    if rc != GPK_OK:
        L = lib()
        raise GpkError("gpk: %s (%d) %s" % (L.gpk_strerror(rc).decode(), rc, L.gpk_last_hip_error().decode()))
    return rc


def stream_ptr(stream):
    """A raw hipStream_t from a torch stream, an int handle or None."""
    return None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)


class _Mem:
    __slots__ = ("__array_interface__",)


def host_view(ptr, count, dtype):
    """A numpy array of `count` elements of `dtype` over library-owned host
    memory at `ptr` (an int or ctypes pointer), without copying. Built from the
    array interface rather than np.ctypeslib.as_array: that creates a ctypes
    array type per distinct length, which ctypes caches for the life of the
    process (about 4.5 KB each), so callbacks that see batches of varying size
    grew the process without bound."""
    dt = np.dtype(dtype)
    if ptr is not None and not isinstance(ptr, int):  # a ctypes pointer or c_void_p
        ptr = ctypes.cast(ptr, ctypes.c_void_p).value
    m = _Mem()
    m.__array_interface__ = {"data": (int(ptr or 0), False), "shape": (int(count),), "version": 3,
                             "typestr": dt.str if dt.fields is None else "|V%d" % dt.itemsize}
    a = np.asarray(m)
    return a if dt.fields is None else a.view(dt)


_synth = None


def synth_lib():
    """libgpk_synth.so: synthetic benchmark batches (bench/test infrastructure)."""
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_PATH):
            raise ImportError("gopacket_amd: %s is not built" % SYNTH_PATH)
        _share_hip_runtime()
        S = ctypes.CDLL(SYNTH_PATH)
        S.gpk_synth_len.argtypes = [ctypes.c_int, ctypes.c_uint64]
        S.gpk_synth_len.restype = ctypes.c_uint32
        S.gpk_synth_fill.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]
        S.gpk_synth_fill.restype = ctypes.c_uint32
        S.gpk_synth_batch_host.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]
        S.gpk_synth_batch_host.restype = ctypes.c_uint64
        S.gpk_synth_device.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        S.gpk_synth_device.restype = ctypes.c_int
        S.gpk_synth_bytes.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
        S.gpk_synth_bytes.restype = ctypes.c_uint64
        S.gpk_synth_write_pcapng.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.c_int]
        S.gpk_synth_write_pcapng.restype = ctypes.c_uint64
        S.gpk_probe_read.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p]
        S.gpk_probe_read.restype = ctypes.c_int
        S.gpk_probe_reread.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p]
        S.gpk_probe_reread.restype = ctypes.c_int
        S.gpk_probe_mixed.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        S.gpk_probe_mixed.restype = ctypes.c_int
        S.gpk_probe_reread_lds.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        S.gpk_probe_reread_lds.restype = ctypes.c_int
        S.gpk_probe_skeleton.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        S.gpk_probe_skeleton.restype = ctypes.c_int
        S.gpk_probe_skeleton_idx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p]
        S.gpk_probe_skeleton_idx.restype = ctypes.c_int
        S.gpk_probe_skeleton_storer.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                                                ctypes.c_void_p]
        S.gpk_probe_skeleton_storer.restype = ctypes.c_int
        S.gpk_probe_malloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64, ctypes.c_uint]
        S.gpk_probe_malloc.restype = ctypes.c_int
        S.gpk_probe_free.argtypes = [ctypes.c_void_p]
        S.gpk_probe_free.restype = ctypes.c_int
        S.gpk_probe_d2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        S.gpk_probe_d2d.restype = ctypes.c_int
        S.gpk_probe_hostwrite.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
        S.gpk_probe_hostwrite.restype = ctypes.c_int
        S.gpk_probe_h2d_rate.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int]
        S.gpk_probe_h2d_rate.restype = ctypes.c_double
        S.gpk_synth_tpacket_v3.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                           ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p]
        S.gpk_synth_tpacket_v3.restype = ctypes.c_uint64
        S.gpk_synth_tp_producer_start.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
        S.gpk_synth_tp_producer_start.restype = ctypes.c_void_p
        S.gpk_synth_tp_producer_stop.argtypes = [ctypes.c_void_p]
        S.gpk_synth_tp_producer_stop.restype = ctypes.c_uint64
        _synth = S
    return _synth
