"""examples/statsassembly.py --device-assembly --flush-older-than against the
timed model (tests/tcpasm_time_model.py): a small generated capture, read in
four batches; before each batch FlushOlderThan(first timestamp - 20 s) runs on
the device, FlushAll at the end. Per stream, in the order of the New calls:
bytes, packets (chunks), skipped, out-of-order, sawStart and sawEnd, and the
(flushed, closed) pair every forced flush logged."""
import pytest

import pcapgen
import pktutil
import tcpasm_model as M
import tcpasm_time_model as TM
import tcpasmtimecases as TT
from configs import oracle_parser
from test_examples_gpu import PARSER, example

pytestmark = pytest.mark.gpu
BATCH, KEEP = 40, 20  # packets per batch; seconds a quiet connection is kept


def test_flush_older_than_example(gpu_ctx, tmp_path):
    pk, _, _ = TT.stream()
    path = str(tmp_path / "stream.pcap")
    with open(path, "wb") as f:
        f.write(pcapgen.pcap_file(pk, nano=True))
    seen = [(1400000000 + i) * 10 ** 9 + i * 7 for i in range(len(pk))]  # pcapgen's timestamps
    data, off, cap = pktutil.pack(pk)
    ref = oracle_parser(PARSER).decode(data, off, cap, layouts=True)
    assert not any(int(r["status"]) & 0x7F for r in ref["records"])  # the loop skips none
    ops = [(p, seen[p] - KEEP * 10 ** 9, True) for p in range(0, len(pk), BATCH)]
    ops.append((len(pk), 1 << 62, True))  # FlushAll: everything is older, CloseAll
    res = TM.run(pk, ref["records"], ref["layouts"], seen, ops)
    want = []
    for st in res["streams"]:
        end, ooo = None, 0
        for ch in st["chunks"]:
            if end is not None and ch["seen"] < end:
                ooo += 1
            else:
                end = ch["seen"]
        want.append([len(st["data"]), len(st["chunks"]), sum(c["skip"] for c in st["chunks"] if c["skip"] > 0), ooo,
                     any(c["flags"] & M.START for c in st["chunks"]), any(c["flags"] & M.END for c in st["chunks"])])
    assert sum(c for _, c in res["flushes"][:-1]) >= 3  # the forced flushes close connections before the end
    logs = []
    streams, read, _ = example().run_device_assembly(path, batch=BATCH, log=logs.append, flush_older_than=KEEP)
    assert read == len(pk)
    got = [[s.bytes, s.packets, s.skipped, s.outOfOrder, s.sawStart, s.sawEnd] for s in streams]
    assert got == want
    assert all(s.complete for s in streams)
    forced = [line for line in logs if line.startswith("forced flush: ")]
    assert forced == ["forced flush: %d flushed, %d closed" % fc for fc in res["flushes"][:-1]]
