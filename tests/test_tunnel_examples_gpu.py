"""examples/detunnel.py over a generated pcapng capture of the tunnel quirk
cases and fuzz packets, in batches of 300: the output file must be the inner
Ethernet frames the model (tunnel_model.py) finds, written by capwrite_model,
with --keep-plain the untunnelled packets too, in capture order."""
import importlib.util
import os

import numpy as np
import pytest

import capwrite_model as W
import configs
import tunnel_model as M
import tunnelcases as C
from pktutil import pack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTF = dict(Name=b"intf0", OS=b"linux", SnapLength=0, LinkType=1, TimestampOffset=0)
SECTION = dict(Hardware=b"amd64", OS=b"linux", Application=b"gopacket")


def example():
    spec = importlib.util.spec_from_file_location("detunnel", os.path.join(ROOT, "examples", "detunnel.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    pk = [p for _, p in C.quirk_cases()[0]] + C.fuzz_packets(C.FUZZ_SEED, 800)
    # every third packet was cut by a snaplen: its Length is larger than what was captured
    meta = [(1700000000 + i // 7, (i * 1000003) % 1000000000, len(p) + (40 if i % 3 == 0 else 0)) for i, p in enumerate(pk)]
    w = W.NgWriter(INTF, SECTION)
    for p, (s, ns, ln) in zip(pk, meta):
        w.write_packet((s, ns), len(p), ln, 0, p)
    path = str(tmp_path_factory.mktemp("detunnel") / "in.pcapng")
    open(path, "wb").write(bytes(w.out))
    data, offs, caps = pack(pk)
    ref = configs.oracle_parser(C.PARSER).decode(data, offs, caps)
    m = M.peel(C.PARSER, data, offs, caps, ref["records"], ref["layouts"], ref["err_args"], gre_checksum=False)
    return path, pk, meta, m


@pytest.mark.parametrize("keep_plain", [False, True], ids=["inner_only", "keep_plain"])
def test_detunnel_writes_the_models_inner_frames(gpu_ctx, tmp_path, capture, keep_plain):
    path, pk, meta, m = capture
    cs = [int(x) for x in m["class_start"]]
    w = W.NgWriter(INTF, SECTION)
    frames = 0
    for i, p in enumerate(pk):
        v = int(m["verdict"][i])
        s, ns, ln = meta[i]
        if cs[0] <= v < cs[1]:
            t = m["tunnels"][v]
            a, k = int(t["inner_off"]), int(t["inner_len"])
            w.write_packet((s, ns), k, max(ln - (len(p) - k), k), 0, p[a:a + k])
        elif v < 0 and keep_plain:
            w.write_packet((s, ns), len(p), ln, 0, p)
        else:
            continue
        frames += 1
    out = str(tmp_path / "out.pcapng")
    read, written = example().run(path, out, keep_plain=keep_plain, batch=300, log=lambda s: None)
    assert (read, written) == (len(pk), frames) and cs[1] - cs[0] > 100
    assert open(out, "rb").read() == bytes(w.out)
    assert np.count_nonzero(m["verdict"] < 0) > 50  # untunnelled packets are among them
