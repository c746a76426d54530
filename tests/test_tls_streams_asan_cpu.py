"""gpk_tls_streams_host under AddressSanitizer + UBSan: the host side of
gopacket_amd/csrc/gpk_tls_streams.hip compiled with the sanitizers into
tests/asan_tls/build/tls_streams_host, a stand-alone program, and run over a
corpus file of every call of tlsstreamcases.py and of a seeded mix. Every
array of a call is a heap block of exactly its size. A sanitizer report or an
output that differs from the model's fails the test. Nothing of it is loaded
into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tlsstream_model as SM
import tlsstreamcases as SC
from gopacket_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ASAN = os.path.join(HERE, "asan_tls")
FILL = 0xA5


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    r = subprocess.run(["make", "-C", ASAN], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(ASAN, "build", "tls_streams_host")


def call_blocks(last, frame_unstarted):
    """The blocks of one recorded call, in the driver's order."""
    data, off, cap, ref = last["arrays"]
    n = len(cap)
    asm = SM.asm_arrays(last["asm"], n)
    carry = [c or (SM.NEW, b"") for c in last["carry"]]
    tails = b"".join(t for _, t in carry)
    offs = np.cumsum([0] + [len(t) for _, t in carry])[:-1] if carry else np.zeros(0)
    want = SM.to_arrays(last["res"], n, fill=FILL)
    scalars = np.array([n, asm["chunk_cap"], asm["data_cap"], len(carry), int(frame_unstarted), FILL], np.uint64)
    return [scalars, np.asarray(data, np.uint8), np.asarray(off, np.uint64), np.asarray(cap, np.uint32),
            np.ascontiguousarray(ref["records"], _lib.RECORD_DTYPE), np.ascontiguousarray(ref["layouts"], _lib.LAYOUT_DTYPE),
            asm["chunks"], asm["stream_first"], asm["stream_closed"], asm["stream_data0"], asm["counts"],
            asm["data"][:asm["data_cap"]], np.array([s for s, _ in carry], np.uint32), np.asarray(offs, np.uint64),
            np.array([len(t) for _, t in carry], np.uint32), np.frombuffer(tails, np.uint8),
            want["streams"], want["recs"], want["hellos"], want["snis"], want["tails"], want["counts"]]


def test_host_side_under_asan(driver, tmp_path):
    cases = SC.cases() + [dict(name="mix", calls=SC.random_mix(7, 200), max_pages=0, frame_unstarted=False, flush=True),
                          dict(name="mix4", calls=SC.random_mix(8, 120), max_pages=4, frame_unstarted=True, flush=True)]
    calls = []
    for case in cases:
        model = SM.Streaming(SC.PARSER, case["max_pages"], case["frame_unstarted"])
        for pk, flush in [(pk, False) for pk in case["calls"]] + ([([], True)] if case["flush"] else []):
            model.feed(pk, flush=flush)
            if model.last is not None:
                calls.append(call_blocks(model.last, case["frame_unstarted"]))
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        f.write(b"TLSS" + struct.pack("<I", len(calls)))
        for blocks in calls:
            for b in blocks:
                raw = np.ascontiguousarray(b).tobytes()
                f.write(struct.pack("<Q", len(raw)) + raw)
    assert len(calls) > 40
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:handle_abort=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([driver, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:],
                                                                                               r.stderr[-4000:])
    assert "tls_streams_host ok: %d calls" % len(calls) in r.stdout
