"""Key derivation at its edges, through gpk_group_batch (key_kernel: the key
from layouts and packet bytes) and gpk_decode_group_batch (derive_key: the key
from the decode kernel's header window in LDS, byte by byte from global memory
past it), against oracle/flows_oracle.py on the decode oracle's results.

The packets (tests/flowcases.py) put addresses, ports, TCP flags and the IPv4
Id before, across and beyond byte 96 of the packet, where the fused kernel's
window ends; neighbouring flows differ in one byte there, so a key word read
wrongly merges or splits groups. The window starts at the packet's offset
rounded down to 16 bytes, so every batch is laid out with the packets at
16-byte multiples plus 0, 1, 2 and 3 (the edge at packet byte 96, 95, 94, 93)
and once packed."""
import numpy as np
import pytest

import flowcases
import pktutil
from flowcheck import Decoded, check_fused, check_group
from gopacket_amd import flows
from oracle import flows_oracle as FO

pytestmark = pytest.mark.gpu

PLACEMENTS = [(16, 0), (16, 1), (16, 2), (16, 3), (1, 0)]


def placed(packets, align, pad):
    """(data, offsets, caplens) with every packet at a multiple of `align`, plus `pad`."""
    if align == 1:
        return pktutil.pack(packets)
    offs, o = [], 0
    for p in packets:
        o = (o + align - 1) // align * align
        offs.append(o + pad)
        o += pad + len(p)
    data = np.zeros(o + 64, np.uint8)
    for q, p in zip(offs, packets):
        data[q:q + len(p)] = np.frombuffer(p, np.uint8)
    return data, np.array(offs, np.uint64), np.array([len(p) for p in packets], np.uint32)


def run(gpu_ctx, packets, kinds):
    """Every placement, every kind, both entry points against the oracle.
    -> {kind: (groups, codes, keys)} of the oracle."""
    g = flows.Grouper(len(packets))
    first = None
    for align, pad in PLACEMENTS:
        P = Decoded(gpu_ctx, packets, batch=placed(packets, align, pad), share=first)
        first = first or P
        for kind in kinds:
            check_group(g, P, kind, what=(align, pad))
            check_fused(g, P, kind, what=(align, pad))
    g.close()
    return {kind: first.oracle(kind) for kind in kinds}


def three_flows_per_layout(codes, n):
    """Every layout's six packets are three groups of two (packets j and j + 3)."""
    for k in range(0, n, 6):
        c = codes[k:k + 6]
        assert min(c) >= 0 and c[0] == c[3] and c[1] == c[4] and c[2] == c[5] and len(set(c)) == 3, (k, c)


def test_window_edge_tcp_ipv4(gpu_ctx):
    cases = flowcases.window_connection4()
    starts = sorted(set(s for s, _ in cases))
    assert starts == list(range(34, 127, 4)) and {82, 86, 90, 94, 98} <= set(starts)
    outs = run(gpu_ctx, [p for _, p in cases], [FO.CONNECTION, FO.DEFRAG])
    three_flows_per_layout(outs[FO.CONNECTION][1], len(cases))


def test_window_edge_addresses_ipv4_in_ipv4(gpu_ctx):
    cases = flowcases.window_connection4in4()
    starts = set(s for s, _ in cases)
    assert {78, 82} <= starts  # destination, source address across byte 96
    assert min(starts) + 20 <= 96 <= max(starts) + 12
    outs = run(gpu_ctx, [p for _, p in cases], [FO.CONNECTION, FO.DEFRAG])
    three_flows_per_layout(outs[FO.CONNECTION][1], len(cases))


def test_window_edge_tcp_ipv6_destination_options(gpu_ctx):
    cases = flowcases.window_connection6()
    starts = set(s for s, _ in cases)
    assert {54 + e for e in (0, 8, 48, 56, 64, 248, 2048)} <= starts
    outs = run(gpu_ctx, [p for _, p in cases], [FO.CONNECTION])
    three_flows_per_layout(outs[FO.CONNECTION][1], len(cases))


def test_window_edge_defrag(gpu_ctx):
    cases = flowcases.window_defrag()
    starts = set(s for s, _ in cases)
    assert {78, 82, 90, 94} <= starts  # destination, source across byte 96; Id before and beyond it
    outs = run(gpu_ctx, [p for _, p in cases], [FO.DEFRAG, FO.CONNECTION])
    three_flows_per_layout(outs[FO.DEFRAG][1], len(cases))


def test_inline_list_boundary(gpu_ctx):
    """TCP as decoded entry 14 and 15 is keyed; from entry 16 on the record's 16
    inline codes do not show it: GPK_GROUP_UNKNOWN."""
    cases = flowcases.inline_boundary_cases()
    outs = run(gpu_ctx, [p for _, p in cases], [FO.CONNECTION, FO.DEFRAG])
    codes = outs[FO.CONNECTION][1]
    want = {"12 tags: IPv4 at 13, TCP at 14": True, "13 tags: IPv4 at 14, TCP at 15": True,
            "14 tags: IPv4 at 15, TCP at 16": False, "15 tags: IPv4 at 16, TCP at 17": False,
            "12 tags, 4in4: TCP at 15": True, "13 tags, 4in4: TCP at 16": False}
    for (label, _), c in zip(cases, codes):
        assert (c >= 0) if want[label] else (c == FO.UNKNOWN), (label, c)


def test_ip_in_ip(gpu_ctx):
    """The last network layer before TCP keys a connection: equal inner
    addresses under different outer ones are one connection, different inner
    ones under equal outer ones are two. DEFRAG looks at the last IPv4 header
    that was decoded: the outer one when it is a fragment (its payload is not
    decoded), else the inner one."""
    cases = flowcases.ip_in_ip_cases()
    outs = run(gpu_ctx, [p for _, p in cases], [FO.CONNECTION, FO.DEFRAG])
    conn = dict(zip([l for l, _ in cases], outs[FO.CONNECTION][1]))
    for name in ("4in4", "6in4", "4in6"):
        base = conn[name + " base"]
        assert base >= 0 and conn[name + " other outer"] == base and conn[name + " base again"] == base
        assert conn[name + " other inner"] >= 0 and conn[name + " other inner"] != base
    assert conn["plain inner"] == conn["4in4 base"] == conn["4in6 base"] != conn["6in4 base"]
    frag = dict(zip([l for l, _ in cases], outs[FO.DEFRAG][1]))
    assert frag["4in4 outer MF, inner DF"] >= 0 and frag["4in4 outer MF, inner DF"] == frag["4in4 outer MF, inner MF"]
    assert frag["4in4 outer DF, inner MF"] >= 0 and frag["4in4 outer DF, inner MF"] == frag["plain inner MF"]
    assert frag["4in4 outer DF, inner MF"] != frag["4in4 outer MF, inner DF"]


def test_useless_filter_at_data_offset_15(gpu_ctx):
    """ACK-only segments whose 40 option bytes fill them are useless, with or
    without Ethernet padding; one payload byte or a SYN keys them. A data
    offset beyond the segment fails the TCP decode (TCP is not in `decoded`),
    so those packets have no key to filter: GPK_GROUP_NONE, as the oracle says."""
    cases = flowcases.useless_filter_cases()
    outs = run(gpu_ctx, [p for _, p in cases] * 2, [FO.CONNECTION, FO.DEFRAG])
    codes = dict(zip([l for l, _ in cases], outs[FO.CONNECTION][1]))
    assert codes["ACK, offset 15, options fill the segment"] == FO.USELESS
    assert codes["the same with Ethernet padding"] == FO.USELESS
    assert codes["ACK, offset 15, one payload byte"] == codes["ACK | SYN, offset 15, no payload"] == 0
    assert codes["ACK, offset 15 in a 20-byte segment"] == FO.NONE
    assert codes["ACK | SYN, offset 15 in a 20-byte segment"] == FO.NONE
    assert codes["ACK, offset 4"] == FO.NONE
