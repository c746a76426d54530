"""gpk_dns_streams_host under AddressSanitizer + UBSan: the host side of
gopacket_amd/csrc/gpk_dns_streams.hip compiled with the sanitizers into
tests/asan_dns/build/dns_streams_host, a stand-alone program with its own main,
and run over a corpus file of every call of dnsstreamcases.py (those on the
cases' default parser, whose port table the program builds), of two seeded
mixes, and of calls with capacities short at either level. Every array of a
call is a heap block of exactly its size. A sanitizer report or an output that
differs from the model's fails the test. Nothing of it is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dnsstream_model as SM
import dnsstreamcases as SC
from dnsstreamutil import mix_case, steps_of
from gopacket_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ASAN = os.path.join(HERE, "asan_dns")
FILL = 0xA5


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    r = subprocess.run(["make", "-C", ASAN], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(ASAN, "build", "dns_streams_host")


def call_blocks(last, frame_unstarted, max_message, caps=(None,) * 4):
    """The blocks of one recorded call, in the driver's order."""
    data, off, cap, ref = last["arrays"]
    n = len(cap)
    asm = SM.asm_arrays(last["asm"], n)
    carry = [c or (SM.NEW, b"") for c in last["carry"]]
    tails = b"".join(t for _, t in carry)
    offs = np.cumsum([0] + [len(t) for _, t in carry])[:-1] if carry else np.zeros(0)
    want = SM.to_arrays(last["res"], n, caps, fill=FILL)
    scalars = np.array([n, asm["chunk_cap"], asm["data_cap"], len(carry), int(frame_unstarted), FILL, max_message],
                       np.uint64)
    return [scalars, np.asarray(data, np.uint8), np.asarray(off, np.uint64), np.asarray(cap, np.uint32),
            np.ascontiguousarray(ref["records"], _lib.RECORD_DTYPE), np.ascontiguousarray(ref["layouts"], _lib.LAYOUT_DTYPE),
            asm["chunks"], asm["stream_first"], asm["stream_closed"], asm["stream_data0"], asm["counts"],
            asm["data"][:asm["data_cap"]], np.array([s for s, _ in carry], np.uint32), np.asarray(offs, np.uint64),
            np.array([len(t) for _, t in carry], np.uint32), np.frombuffer(tails, np.uint8),
            want["streams"], want["msgs"], want["rrs"], want["names"], want["tails"], want["counts"]]


def test_host_side_under_asan(driver, tmp_path):
    cases = [c for c in SC.cases() if c["parser"] is SC.PARSER]
    cases += [mix_case(SC.random_mix(7, 200)), mix_case(SC.random_mix(8, 120), max_pages=4, frame_unstarted=True),
              mix_case(SC.random_mix(9, 120), max_message=40)]
    calls = []
    for case in cases:
        model = SM.Streaming(SC.PARSER, case["max_pages"], case["frame_unstarted"], case["max_message"])
        for pk, flush in steps_of(case):
            model.feed(pk, flush=flush)
            if model.last is None:
                continue
            calls.append(call_blocks(model.last, case["frame_unstarted"], case["max_message"]))
            if case["name"] in ("mix", "messages_65", "split_two_calls"):  # short at level one, then at level two
                full = SM.to_arrays(model.last["res"], len(model.last["arrays"][2]))
                need = [len(full[k]) for k in ("msgs", "rrs", "names", "tails")]
                for caps in ([x // 2 for x in need], [need[0], need[1] // 2, need[2] // 3, need[3]], [0, 0, 0, 0]):
                    calls.append(call_blocks(model.last, case["frame_unstarted"], case["max_message"], caps))
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        f.write(b"DNSS" + struct.pack("<I", len(calls)))
        for blocks in calls:
            for b in blocks:
                raw = np.ascontiguousarray(b).tobytes()
                f.write(struct.pack("<Q", len(raw)) + raw)
    assert len(calls) > 60
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:handle_abort=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([driver, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:],
                                                                                               r.stderr[-4000:])
    assert "dns_streams_host ok: %d calls" % len(calls) in r.stdout
