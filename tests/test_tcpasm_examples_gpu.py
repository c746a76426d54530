"""examples/statsassembly.py --device-assembly (tcpassembly on the device through
gopacket_amd.tcpassembly) against the reassembly model: the capture reader
oracle's packets that the decode oracle decodes without error (the loop skips
the others, main.go:179-182), run through tests/tcpasm_model.py with FlushAll
at the end. Per stream, in the order of the New calls: bytes, packets (chunks),
skipped, out-of-order (by the capture time of each chunk's source packet),
sawStart and sawEnd; every stream is complete after the flush. The file is
read in several batches, so the streaming state carries connections across."""
import os

import numpy as np
import pytest

import tcpasm_model as M
from configs import oracle_parser
from oracle import pcapgo_oracle as PO
from test_examples_gpu import PARSER, ROOT, example

pytestmark = pytest.mark.gpu


def expected(path, max_pages):
    raw = open(path, "rb").read()
    r = PO.read_all(raw, kind="ng" if raw[:4] == b"\x0a\x0d\x0d\x0a" else "pcap")
    s = r["stream"]
    pk = [bytes(s[p.offset:p.offset + p.caplen]) for p in r["packets"]]
    ts = [p.ts_sec + p.ts_nsec * 1e-9 for p in r["packets"]]
    cap = np.array([len(p) for p in pk], np.uint32)
    off = np.zeros(len(pk), np.uint64)
    off[1:] = np.cumsum(cap[:-1], dtype=np.uint64)
    ref = oracle_parser(PARSER).decode(np.frombuffer(b"".join(pk) + bytes(16), np.uint8), off, cap, layouts=True)
    ok = [i for i in range(len(pk)) if not int(ref["records"][i]["status"]) & 0x7F]
    res = M.run([pk[i] for i in ok], [ref["records"][i] for i in ok], [ref["layouts"][i] for i in ok],
                max_pages=max_pages, flush=True)
    out = []
    for st in res["streams"]:
        end, ooo = None, 0
        for ch in st["chunks"]:
            seen = ts[ok[ch["src"]]]
            if end is not None and seen < end:
                ooo += 1
            else:
                end = seen
        out.append([len(st["data"]), len(st["chunks"]), sum(c["skip"] for c in st["chunks"] if c["skip"] > 0), ooo,
                    any(c["flags"] & M.START for c in st["chunks"]), any(c["flags"] & M.END for c in st["chunks"])])
    return out, len(pk), res["log"]


@pytest.mark.parametrize("src,max_pages", [("c6_pcapng", 0), ("c6_pcapng", 2), ("test_ethernet_pcap", 0)])
def test_device_assembly_example(gpu_ctx, tmp_path, src, max_pages):
    from gopacket_amd import _lib
    if src == "c6_pcapng":
        path = str(tmp_path / "c6.pcapng")
        assert _lib.synth_lib().gpk_synth_write_pcapng(path.encode(), 6, 0, 12000, 4) > 0
    else:
        path = os.path.join(ROOT, "tests", "golden", "test_ethernet.pcap")
    want, n, _ = expected(path, max_pages)
    logs = []
    streams, read, _ = example().run_device_assembly(path, batch=2500, max_pages=max_pages, log=logs.append)
    assert read == n
    got = [[s.bytes, s.packets, s.skipped, s.outOfOrder, s.sawStart, s.sawEnd] for s in streams]
    assert got == want, (len(got), len(want))
    assert all(s.complete for s in streams)
    assert len(want) > (100 if src == "c6_pcapng" else 0)
    assert sum(line.startswith("new stream ") for line in logs) == len(want)
    assert sum(line.startswith("Reassembly of stream ") for line in logs) == len(want)
    assert logs[-1].startswith("processed ")
