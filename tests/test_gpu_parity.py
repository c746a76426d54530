"""Device (HIP, through the C ABI) vs oracle parity. Bit-exact: every record
field, error argument, flow hash and layer layout must be identical.

All packets are built here; nothing reads /root/reference at run time.
"""
import struct
import zlib

import numpy as np
import pytest

import pktutil
from configs import CONFIGS, assert_same, device_parser, oracle_parser

pytestmark = pytest.mark.gpu


def golden_packets():
    g = pktutil.golden()
    pk = [bytes.fromhex(v["hex"]) for k, v in sorted(g.items()) if "hex" in v]
    for name in ("test_ethernet.pcap", "test_dns.pcap"):
        pk += pktutil.read_pcap(pktutil.GOLDEN + "/" + name)[1]
    sll = bytes.fromhex(g["mptcp_bad_len_sll2"]["hex"])
    pk.append(sll[20:])  # the IPv4 packet inside the Linux SLL2 header
    return pk


def run_both(ctx, cfg, packets, align=1, pad=0, layouts=True):
    data, off, cap = pktutil.pack(packets, align=align, pad=pad)
    dev = ctx.decode_host(device_parser(cfg), data, off, cap, layouts=layouts)
    ref = oracle_parser(cfg).decode(data, off, cap, nthreads=8, layouts=layouts)
    return dev, ref


@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_golden_packets(gpu_ctx, cfg_name):
    dev, ref = run_both(gpu_ctx, CONFIGS[cfg_name], golden_packets())
    assert_same(dev, ref, cfg_name)


@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
@pytest.mark.parametrize("align", [1, 16])
def test_fuzz(gpu_ctx, cfg_name, align):
    packets = pktutil.fuzz_packets(zlib.crc32(cfg_name.encode()) % 1000 + align, 40000)
    dev, ref = run_both(gpu_ctx, CONFIGS[cfg_name], packets, align=align, pad=align // 2)
    assert_same(dev, ref, cfg_name)
    # the same packets through the kernels without layout output (the small-packet
    # specialisations: dword-aligned 5-chunk window for parsers without IPv6, else 6 chunks)
    data, off, cap = pktutil.pack(packets, align=align, pad=align // 2)
    dev2 = gpu_ctx.decode_host(device_parser(CONFIGS[cfg_name]), data, off, cap, layouts=False)
    assert_same(dev2, ref, cfg_name + " (no layouts)")
    err = dev["records"]["status"] & 0x7F
    if cfg_name != "first_unregistered":  # that one fails every packet with UnsupportedLayerType(LLC)
        assert len(np.unique(err)) > 5  # the fuzzer reaches many error sites


@pytest.mark.parametrize("synth_cfg,cfg_name", [(2, "eth_ip4_udp_payload"), (3, "eth_ip4_tcp_payload"),
                                                (4, "statsassembly")])
def test_synthetic(gpu_ctx, synth_cfg, cfg_name):
    from gopacket_amd import synth
    data, off, cap = synth.host_batch(synth_cfg, 123456789, 100000)
    dev = gpu_ctx.decode_host(device_parser(CONFIGS[cfg_name]), data, off, cap, layouts=True)
    ref = oracle_parser(CONFIGS[cfg_name]).decode(data, off, cap, nthreads=8)
    assert_same(dev, ref, "synth%d" % synth_cfg)


@pytest.mark.parametrize("synth_cfg,want", [
    (2, "gpk::decode_kernel<true,false,true,false,5,7,4>"),  # 64-76 B: the dword-aligned 5-chunk kernel
    (4, "gpk::decode_sb_kernel<true,7,6,false>"),            # IMIX, mean 362 B: stream before the parse
    (3, "gpk::decode_kernel<true,false,true,false,6,6,16>"),  # 1500 B: the 80-VGPR 6-chunk kernel
], ids=["synth2-small", "synth4-stream", "synth3-big"])  # ids without "::", which pytest node ids split at
def test_kernel_choice_by_mean_packet(gpu_ctx, synth_cfg, want):
    """A parser without IPv6 (Ethernet, IPv4, TCP, Payload) takes the kernel
    its batch's mean packet selects (GPK_MID_MAXMEAN = 256 B, big packets from
    1 KiB); each gives the oracle's results on the same packets (tagged, IPv6
    and UDP packets end in UnsupportedLayerType, as DecodeLayers does)."""
    from gopacket_amd import synth
    cfg = CONFIGS["eth_ip4_tcp_payload"]
    data, off, cap = synth.host_batch(synth_cfg, 99, 40000)
    dp = device_parser(cfg)
    assert gpu_ctx.kernel_name(dp, data, off, cap, layouts=False) == want
    dev = gpu_ctx.decode_host(dp, data, off, cap, layouts=False)
    ref = oracle_parser(cfg).decode(data, off, cap, nthreads=8, layouts=False)
    assert_same(dev, ref, "synth%d through %s" % (synth_cfg, want))


def unsupported_type_packets():
    """Packets whose decode ends at an EtherType or IPProtocol with no
    registered decoder in some configs (ARP, LLDP, an unknown EtherType, ICMP,
    GRE, ICMPv6, an unassigned protocol, IPv6 behind tags), each at several
    payload lengths and behind 0, 1 and 2 VLAN tags."""
    mac = b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02"

    def ip4(proto, payload):
        h = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 20 + len(payload), 7, 0, 64, proto, 0, b"\x0a\x00\x00\x01",
                        b"\x0a\x00\x00\x02")
        return h + payload

    def ip6(nh, payload):
        return struct.pack(">IHBB16s16s", 6 << 28, len(payload), nh, 64, b"\x20\x01" + b"\x00" * 13 + b"\x01",
                           b"\x20\x01" + b"\x00" * 13 + b"\x02") + payload

    bodies = []
    for n in (1, 8, 28, 46):
        pay = bytes(range(n))
        bodies += [(0x0806, pay), (0x88CC, pay), (0x9999, pay), (0x0800, ip4(1, pay)), (0x0800, ip4(47, pay)),
                   (0x0800, ip4(253, pay)), (0x0800, ip4(6, b"")), (0x86DD, ip6(58, pay)), (0x86DD, ip6(59, pay))]
    out = []
    for et, body in bodies:
        for tags in (b"", struct.pack(">HH", 0x8100, 5), struct.pack(">HHHH", 0x88A8, 5, 0x8100, 6)):
            if tags:
                out.append(mac + tags[:2] + tags[2:] + struct.pack(">H", et) + body)
            else:
                out.append(mac + struct.pack(">H", et) + body)
    return out


@pytest.mark.parametrize("layouts", [False, True])
@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_unsupported_types(gpu_ctx, cfg_name, layouts):
    """DecodeLayers stops with UnsupportedLayerType (or without an error for
    LayerTypeZero, or with IgnoreUnsupported) at a type no decoder handles
    (layers_decoder.go:71-79): the lanes the fast path hands to the general
    decoder there give the oracle's results, in every test parser."""
    pk = unsupported_type_packets() * 3
    dev, ref = run_both(gpu_ctx, CONFIGS[cfg_name], pk, layouts=layouts)
    assert_same(dev, ref, "%s unsupported types (layouts=%s)" % (cfg_name, layouts))
    if cfg_name == "eth_ip4_tcp_payload":
        err = dev["records"]["status"] & 0x7F
        assert len(np.unique(err)) >= 2


def test_edge_sizes(gpu_ctx):
    """Empty packets, 1-byte packets, a jumbogram larger than 64 KiB and the
    snaplen maximum, at odd offsets."""
    g = pktutil.golden()
    base = bytes.fromhex(g["simple_tcp"]["hex"])
    jumbo = bytearray(base)
    jumbo += bytes(np.random.default_rng(1).integers(0, 256, 70000, dtype=np.uint8))
    # IPv4 Length 0 (TSO): length becomes uint16(len(data)) (ip4.go:189-193)
    jumbo[16:18] = b"\x00\x00"
    big = bytearray(base) + bytes(262144 - len(base))
    big[16:18] = b"\x00\x00"
    # the IPv6 UDP jumbogram of tcpip_test.go:138-186 (its UDP decode fails under
    # DecodeLayers) and the variant whose UDP segment of 65 560 bytes is
    # summed, with the pseudo-header's length>>16 term (raw_ip6 config)
    j6 = [pktutil.ipv6_udp_jumbogram(0xcda8), pktutil.ipv6_udp_jumbogram(hbh16=True)]
    packets = [b"", b"\x00", base[:13], base[:14], base, bytes(jumbo), bytes(big), base[:60]] * 3 + j6
    for name in sorted(CONFIGS):
        dev, ref = run_both(gpu_ctx, CONFIGS[name], packets, align=1, pad=3)
        assert_same(dev, ref, name)


def test_error_text(gpu_ctx):
    """gpk_format_error renders the same Go text as the oracle for every error the fuzzer produced."""
    from gopacket_amd import engine
    cfg = CONFIGS["statsassembly"]
    dev, _ = run_both(gpu_ctx, cfg, pktutil.fuzz_packets(7, 20000))
    op = oracle_parser(cfg)
    st = dev["records"]["status"]
    seen = set()
    for i in np.nonzero(st & 0x7F)[0]:
        code = int(st[i] & 0x7F)
        a0, a1 = int(dev["err_args"][2 * i]), int(dev["err_args"][2 * i + 1])
        if (code, a0, a1) in seen:
            continue
        seen.add((code, a0, a1))
        assert engine.format_error(code, a0, a1) == op.error_string(code, a0, a1)
    assert len(seen) > 10


def test_long_decoded_lists(gpu_ctx):
    """Lists longer than the 16 inline codes: stacked 802.1Q tags and IPv4-in-IPv4."""
    import struct
    cfg = CONFIGS["statsassembly"]
    pkts = []
    for ntags in (15, 16, 17, 40):
        hdr = b"\x02" * 12 + struct.pack(">H", 0x8100)
        tags = b"".join(struct.pack(">HH", 1, 0x8100) for _ in range(ntags - 1)) + struct.pack(">HH", 1, 0x0800)
        ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 20 + 8, 0, 0, 64, 17, 0, b"\x01" * 4, b"\x02" * 4)
        pkts.append(hdr + tags + ip + struct.pack(">HHHH", 1234, 5678, 8, 0))
    ip_chain = b""
    for k in range(20):
        ip_chain = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 20 + len(ip_chain) + (0 if k else 8), 0, 0, 64,
                               4 if k else 17, 0, b"\x01" * 4, b"\x02" * 4) + ip_chain + (b"" if k else b"\x00" * 8)
    pkts.append(b"\x02" * 12 + b"\x08\x00" + ip_chain)
    dev, ref = run_both(gpu_ctx, cfg, pkts)
    assert_same(dev, ref, "long lists")
    dp, op = device_parser(cfg), oracle_parser(cfg)
    for p in pkts:
        assert gpu_ctx.decoded_list_host(dp, p) == op.decoded_list(p)


def test_device_resident_matches_host(gpu_ctx):
    """gpk_decode_batch on torch device tensors == gpk_decode_batch_host."""
    import torch
    from gopacket_amd import _lib, synth
    cfg = CONFIGS["statsassembly"]
    p = device_parser(cfg)
    n = 50000
    data, off, cap = synth.device_batch(4, 5, n)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    lay = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(p, data, off, cap, rec, err, fl, lay, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    hd, ho, hc = synth.host_batch(4, 5, n)
    assert np.array_equal(data.cpu().numpy()[:len(hd) - 16], hd[:len(hd) - 16])
    host = gpu_ctx.decode_host(p, hd, ho, hc, layouts=True)
    dev = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
               flows=fl.cpu().numpy().view(np.uint64), layouts=lay.cpu().numpy().view(_lib.LAYOUT_DTYPE))
    assert_same(dev, host, "device vs host")


@pytest.mark.parametrize("outputs", [0, 1, 2, 4, 3, 5, 6, 7])
@pytest.mark.parametrize("synth_cfg,cfg_name", [(2, "eth_ip4_udp_payload"), (4, "statsassembly")])
def test_output_selection(gpu_ctx, outputs, synth_cfg, cfg_name):
    """Every GPK_OUT_* subset (each selects a different kernel specialisation)."""
    from gopacket_amd import synth
    cfg = dict(CONFIGS[cfg_name], outputs=outputs)
    data, off, cap = synth.host_batch(synth_cfg, 1000, 20000)
    for layouts in (False, True):
        dev = gpu_ctx.decode_host(device_parser(cfg), data, off, cap, layouts=layouts)
        ref = oracle_parser(cfg).decode(data, off, cap, nthreads=8, layouts=layouts)
        if not outputs & 4:
            dev["flows"][:] = 0
        assert_same(dev, ref, "outputs=%d layouts=%s" % (outputs, layouts))


def test_new_parser_after_free_uploads_its_tables(gpu_ctx):
    """A parser created after another was freed (possibly at the same address,
    with the same number of changes) must not reuse the freed one's tables."""
    import gc
    from gopacket_amd import synth
    data, off, cap = synth.host_batch(2, 0, 5000)
    a = device_parser(CONFIGS["eth_ip4_tcp_payload"])
    gpu_ctx.decode_host(a, data, off, cap)
    del a
    gc.collect()
    for _ in range(4):
        b = device_parser(CONFIGS["eth_ip4_udp_payload"])
        dev = gpu_ctx.decode_host(b, data, off, cap)
        ref = oracle_parser(CONFIGS["eth_ip4_udp_payload"]).decode(data, off, cap, layouts=False)
        assert_same(dev, ref, "fresh parser")
        del b
        gc.collect()


@pytest.mark.parametrize("base", [(1 << 31) - 700, (1 << 32) + 3, (5 << 30) + 8])
def test_offsets_beyond_2_and_4_GiB(gpu_ctx, base):
    """Packets placed past 2 GiB / 4 GiB in a device buffer (64-bit offsets end to end)."""
    import torch
    from gopacket_amd import _lib, synth
    cfg = CONFIGS["statsassembly"]
    hd, ho, hc = synth.host_batch(4, 77, 20000)
    hd3, ho3, hc3 = synth.host_batch(3, 77, 4000)
    data = torch.zeros(base + len(hd) + len(hd3) + 4096, dtype=torch.uint8, device="cuda")
    data[base:base + len(hd)] = torch.from_numpy(hd).cuda()
    b3 = base + len(hd)
    data[b3:b3 + len(hd3)] = torch.from_numpy(hd3).cuda()
    off = np.concatenate([ho + base, ho3 + b3]).astype(np.int64)
    cap = np.concatenate([hc, hc3]).astype(np.int32)
    n = len(off)
    rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    fl = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    gpu_ctx.decode_device(device_parser(cfg), data, torch.from_numpy(off).cuda(), torch.from_numpy(cap).cuda(),
                          rec, err, fl, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    pk = [bytes(hd[o:o + c]) for o, c in zip(ho, hc)] + [bytes(hd3[o:o + c]) for o, c in zip(ho3, hc3)]
    rd, ro, rc = pktutil.pack(pk)
    ref = oracle_parser(cfg).decode(rd, ro, rc, layouts=False)
    dev = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE), err_args=err.cpu().numpy().view(np.uint32),
               flows=fl.cpu().numpy().view(np.uint64), layouts=None)
    assert_same(dev, ref, "base %d" % base)
    del data
    torch.cuda.empty_cache()


@pytest.mark.parametrize("cfg_name", ["statsassembly", "overrides", "many_ports", "tables_overflow", "raw_ip6",
                                      "first_unregistered"])
def test_global_table_mode(gpu_ctx, cfg_name):
    """GPK_TABLES_GLOBAL (full tables in device memory) gives the same results
    as the oracle, like the default compact LDS tables do."""
    from gopacket_amd import _lib
    gpu_ctx.set_table_mode(_lib.TABLES_GLOBAL)
    try:
        packets = golden_packets() + pktutil.fuzz_packets(zlib.crc32(cfg_name.encode()) % 1000 + 5, 20000)
        dev, ref = run_both(gpu_ctx, CONFIGS[cfg_name], packets)
        assert_same(dev, ref, cfg_name + " global tables")
    finally:
        gpu_ctx.set_table_mode(_lib.TABLES_AUTO)


def test_port_traffic_hits_table_entries(gpu_ctx):
    """Packets whose ports/ethertypes are exactly the keys stored in the
    compact hash tables (every probe depth) decode like the oracle."""
    import struct
    cfg = CONFIGS["many_ports"]
    pk = []
    for port in list(cfg["tcp_port"]) + [0, 65535, 65534, 101, 4096]:
        ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 40, 0, 0, 64, 6, 0, b"\x01" * 4, b"\x02" * 4)
        for sp, dp in ((port, 9), (9, port), (port, port)):
            tcp = struct.pack(">HHIIBBHHH", sp, dp, 1, 2, 0x50, 0x18, 100, 0, 0)
            pk.append(b"\x02" * 12 + b"\x08\x00" + ip + tcp + b"xyz")
    for port in list(cfg["udp_port"]) + [53, 4789, 65535, 0]:
        ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 31, 0, 0, 64, 17, 0, b"\x01" * 4, b"\x02" * 4)
        pk.append(b"\x02" * 12 + b"\x08\x00" + ip + struct.pack(">HHHH", port, 7, 11, 0) + b"abc")
    dev, ref = run_both(gpu_ctx, cfg, pk)
    assert_same(dev, ref, "many_ports keys")


def phase_b_layout(packets, layout):
    """The packets of `packets` placed in one buffer as `layout` says:
    sparse4k   every packet at a multiple of 4 KiB (sparse waves)
    sparse_mix packed, but every 8th packet moved to a 4 KiB-aligned place past
               the packed ones (mean packet still under 1 KiB: the small-packet
               kernels, whose waves are then not packed)
    gapped     in order, 1-40 random bytes between packets (the tail granule of
               a segment is never the next packet's first bytes)
    shuffled / reversed            the packed buffer's index permuted / reversed
    wave_shuffled                  permuted inside each group of 64 (a wave's
                                   region is compact, its packets out of order)"""
    rng = np.random.default_rng(9)
    if layout == "sparse4k":
        return pktutil.pack(packets, align=4096)
    if layout == "gapped":
        offs, o = [], 0
        for p in packets:
            o += int(rng.integers(1, 41))
            offs.append(o)
            o += len(p)
        data = np.zeros(o + 64, np.uint8)
        for q, p in zip(offs, packets):
            data[q:q + len(p)] = np.frombuffer(p, np.uint8) if len(p) else []
        return data, np.array(offs, np.uint64), np.array([len(p) for p in packets], np.uint32)
    if layout == "sparse_mix":
        data, off, cap = pktutil.pack(packets)
        far = np.arange(len(packets)) % 8 == 5
        end = (len(data) + 4095) // 4096 * 4096
        new_off = off.copy()
        new_off[far] = end + 4096 * np.arange(far.sum(), dtype=np.uint64) + np.uint64(3)
        big = np.zeros(int(new_off[far][-1]) + 4096 + 64, np.uint8)
        big[:len(data)] = data
        for q, o, c in zip(new_off[far], off[far], cap[far]):
            big[int(q):int(q) + int(c)] = data[int(o):int(o) + int(c)]
        return big, new_off, cap
    data, off, cap = pktutil.pack(packets)
    order = np.arange(len(packets))
    if layout == "shuffled":
        order = rng.permutation(len(packets))
    elif layout == "reversed":
        order = order[::-1].copy()
    elif layout == "wave_shuffled":
        for k in range(0, len(order), 64):
            order[k:k + 64] = rng.permutation(order[k:k + 64])
    return data, off[order], cap[order]


# the kernels the no-layout runs must take (gpk_decode_kernel_name): the
# stream-before-parse kernel for parsers with IPv6, the dword-aligned 5-chunk
# kernel for parsers without when the batch's mean (buffer bytes / packets) is
# under 256 B (GPK_MID_MAXMEAN; the stream-before-parse kernel from there on);
# batches with a mean packet of 1 KiB or more take the 80-VGPR 6-chunk kernel
SB_KERNEL = "gpk::decode_sb_kernel<true,7,6,false>"
PHASE_B_KERNELS = {
    "statsassembly": SB_KERNEL,
    "raw_ip6": SB_KERNEL,
    "eth_ip4_tcp_payload": "gpk::decode_kernel<true,false,true,false,5,7,4>",
}


def phase_b_kernel(name, data, off):
    mean = len(data) // max(1, len(off))
    if mean >= 1024:
        return "gpk::decode_kernel<true,false,true,false,6,6,16>"
    if name == "eth_ip4_tcp_payload" and mean >= 256:
        return SB_KERNEL
    return PHASE_B_KERNELS[name]


@pytest.mark.parametrize("layouts", [True, False])
@pytest.mark.parametrize("layout", ["sparse4k", "sparse_mix", "gapped", "shuffled", "reversed", "wave_shuffled"])
def test_phase_b_layouts(gpu_ctx, layout, layouts):
    """The L4 segment sums take the dense prefix stream when a wave's segments
    share a compact region and the per-segment stream otherwise: sparse,
    gapped, shuffled and reversed layouts must all give the oracle's results
    (layers_decoder.go:60-79 and tcpip.go:54-69 on packets at arbitrary
    offsets, include/gpk.h gpk_batch), through the layout kernel and through
    the default small-packet kernels (their next-lane tail rules and their
    fallbacks when a wave's packets are not packed)."""
    packets = pktutil.fuzz_packets(4242, 12000) + golden_packets()
    data, off, cap = phase_b_layout(packets, layout)
    for name in ("statsassembly", "eth_ip4_tcp_payload", "raw_ip6"):
        cfg = CONFIGS[name]
        dp = device_parser(cfg)
        if not layouts:
            want = phase_b_kernel(name, data, off)
            assert gpu_ctx.kernel_name(dp, data, off, cap, layouts=False) == want, (layout, name)
        dev = gpu_ctx.decode_host(dp, data, off, cap, layouts=layouts)
        ref = oracle_parser(cfg).decode(data, off, cap, nthreads=8, layouts=layouts)
        assert_same(dev, ref, "%s/%s/layouts=%s" % (layout, name, layouts))


# ---- kernel selection, pinned -------------------------------------------------
# The 12 specialisations select() can answer with (gpk_kernels.hip kKernels), as
# gpk_decode_kernel_name prints them; %s is the table mode ("true": compact LDS
# tables, "false": GPK_TABLES_GLOBAL).
K_BIG = "gpk::decode_kernel<true,false,%s,false,6,6,16>"
K_BIG_NOL4 = "gpk::decode_kernel<false,false,%s,false,6,6,16>"
K_LAY = "gpk::decode_kernel<true,true,%s,false,6,6,16>"
K_LAY_NOL4 = "gpk::decode_kernel<false,true,%s,false,6,6,16>"
K_W4 = "gpk::decode_kernel<false,false,%s,false,4,6,16>"
K_W5 = "gpk::decode_kernel<true,false,%s,false,5,7,4>"
K_W5_NOL4 = "gpk::decode_kernel<false,false,%s,false,5,7,4>"
K_SMALL_NOL4 = "gpk::decode_kernel<false,false,%s,false,6,7,16>"
K_SB = "gpk::decode_sb_kernel<%s,7,6,false>"
K_FIELDS = "gpk::decode_sb_kernel<%s,5,6,true>"
# (with fused grouping keys: decode_kernel<l4,false,%s,true,6,6,16>, which the C
# ABI has no name query for; those launches are checked by their results)

# parser -> batch (synthetic config: mean packet) -> kernel without layouts for
# (L4 checksum on, off). With layouts every parser and batch takes K_LAY /
# K_LAY_NOL4, the fused fields launch K_FIELDS.
SELECTION_PARSERS = {
    "eth_ip4_udp_payload": "header-only: no Dot1Q/IPv6/TCP decoder (4-chunk window without the L4 checksum)",
    "eth_ip4_tcp_payload": "no IPv6 decoder (dword-aligned 5-chunk window under GPK_MID_MAXMEAN = 256 B)",
    "statsassembly": "full parser",
}
SELECTION_BATCHES = {2: (0, 256), 4: (256, 1024), 3: (1024, 1 << 20)}  # synth config: its mean packet's band, bytes
SELECTION = {
    "eth_ip4_udp_payload": {2: (K_W5, K_W4), 4: (K_SB, K_W4), 3: (K_BIG, K_W4)},
    "eth_ip4_tcp_payload": {2: (K_W5, K_W5_NOL4), 4: (K_SB, K_SMALL_NOL4), 3: (K_BIG, K_BIG_NOL4)},
    "statsassembly": {2: (K_SB, K_SMALL_NOL4), 4: (K_SB, K_SMALL_NOL4), 3: (K_BIG, K_BIG_NOL4)},
}
SELECTION_N = 257  # two workgroups, the second with one active lane: inactive-lane prologue and a partial wave
_selection_cache = {}


def selection_case(name, synth_cfg, l4):
    """The 257-packet batch of a synthetic config and the oracle's results for
    it (with and without layouts), computed once per parser, batch and outputs."""
    from gopacket_amd import synth
    key = (name, synth_cfg, l4)
    if key not in _selection_cache:
        if ("batch", synth_cfg) not in _selection_cache:
            _selection_cache["batch", synth_cfg] = synth.host_batch(synth_cfg, 31, SELECTION_N)
        data, off, cap = _selection_cache["batch", synth_cfg]
        cfg = dict(CONFIGS[name], outputs=7 if l4 else 5)  # GPK_OUT_L4_CSUM = 2
        op = oracle_parser(cfg)
        _selection_cache[key] = (cfg, data, off, cap, op.decode(data, off, cap, nthreads=1, layouts=True),
                                 op.decode(data, off, cap, nthreads=1, layouts=False))
    return _selection_cache[key]


@pytest.mark.parametrize("tables", ["compact", "global"])
def test_selection_is_pinned(gpu_ctx, tables):
    """Every selection input (L4 checksum, layouts / fused fields / fused keys,
    the parser's header class, the batch's mean packet, the table mode) takes
    the kernel named here, that kernel is resident at least once per CU, and
    257 packets through it give the oracle's results bit for bit."""
    import torch
    from gopacket_amd import _lib, flows
    mode = "true" if tables == "compact" else "false"
    grouper = flows.Grouper(SELECTION_N)
    gpu_ctx.set_table_mode(_lib.TABLES_GLOBAL if tables == "global" else _lib.TABLES_AUTO)
    try:
        for name in SELECTION_PARSERS:
            for synth_cfg, (lo, hi) in SELECTION_BATCHES.items():
                for l4 in (True, False):
                    cfg, data, off, cap, ref_lay, ref = selection_case(name, synth_cfg, l4)
                    assert len(off) == SELECTION_N and lo <= len(data) // len(off) < hi
                    dp = device_parser(cfg)
                    what = "%s/synth%d/l4=%s/%s" % (name, synth_cfg, l4, tables)
                    plain = SELECTION[name][synth_cfg][0 if l4 else 1]
                    for layouts, want in ((False, plain), (True, K_LAY if l4 else K_LAY_NOL4),
                                          (_lib.NAME_FIELDS, K_FIELDS)):
                        assert gpu_ctx.kernel_name(dp, data, off, cap, layouts=layouts) == want % mode, (what, layouts)
                        assert gpu_ctx.occupancy(dp, data, off, cap, layouts=layouts) >= 1, (what, layouts)
                        if layouts == _lib.NAME_FIELDS:
                            dev = gpu_ctx.decode_host(dp, data, off, cap, layouts=False, fields=True)
                        else:
                            dev = gpu_ctx.decode_host(dp, data, off, cap, layouts=layouts)
                        assert_same(dev, ref_lay if layouts is True else ref, "%s/layouts=%s" % (what, layouts))
                    # fused grouping keys (gpk_decode_group_batch): the decode's own outputs
                    d = torch.from_numpy(data).cuda()
                    o = torch.from_numpy(off.astype(np.int64)).cuda()
                    c = torch.from_numpy(cap.astype(np.int32)).cuda()
                    rec = torch.zeros(SELECTION_N * 16, dtype=torch.uint8, device="cuda")
                    err = torch.zeros(2 * SELECTION_N, dtype=torch.int32, device="cuda")
                    fl = torch.zeros(3 * SELECTION_N, dtype=torch.int64, device="cuda")
                    grouper.decode_group(gpu_ctx, dp, d, o, c, rec, err, fl, kind=flows.CONNECTION)
                    torch.cuda.synchronize()
                    dev = dict(records=rec.cpu().numpy().view(_lib.RECORD_DTYPE),
                               err_args=err.cpu().numpy().view(np.uint32), flows=fl.cpu().numpy().view(np.uint64),
                               layouts=None)
                    assert_same(dev, ref, what + "/keys")
    finally:
        gpu_ctx.set_table_mode(_lib.TABLES_AUTO)
        grouper.close()
