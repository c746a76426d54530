"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the headline config's
timed steps and the result line, nothing that --full adds; and --dump-outputs,
whose files hold the last step's outputs for the documented packet sample,
value for value what the oracle computes for those packets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dumped_outputs(tmp_path):
    import bench
    from gopacket_amd import synth
    from oracle import oracle as O
    n = bench.DUMP_PACKETS + 857  # more than one dump holds: the sampled form
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--packets", str(n),
           "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["full"] is False and r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1
    assert r["unit"] == "Mpkts/s" and r["higher_is_better"] is True and r["dtype"] == "u8"
    assert r["ms_per_step"] > 0
    # value = packets per timed step / ms_per_step (ms_per_step is rounded to 0.1 us, a step here takes tens of us)
    assert r["value"] == pytest.approx(n / r["ms_per_step"] / 1e3, rel=1e-2)
    assert r["config"]["packets_per_gpu"] == n and r["roofline"]["kernel"].startswith("gpk::decode_kernel<")
    # nothing that takes a run of its own
    assert r["configs"] == {} and r["parity"] is None and r["full_parity"] is None and r["narrow"] is None
    assert r["cpu_baseline"] is None and r["roofline"]["probe_read_GBps"] is None
    assert r["roofline"]["skeleton_ms"] is None
    assert not {"fields", "c5", "pcie_inclusive", "bpf", "flows", "afpacket"} & set(r)

    rng = np.random.default_rng(20)
    idx = np.unique(np.concatenate([rng.integers(0, n, bench.DUMP_PACKETS), [0, n - 1]]))
    k = len(idx)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["err_args", "flows", "records"]
    assert got["records"].dtype == np.float32 and got["records"].shape == (k, 16)
    assert got["err_args"].dtype == np.float64 and got["err_args"].shape == (k, 2)
    assert got["flows"].dtype == np.float32 and got["flows"].shape == (k, 24)
    assert sum(a.nbytes for a in got.values()) <= 64e6
    cfg = bench.CONFIGS["c3"]
    hd, ho, hc = synth.host_batch(cfg["synth"], 0, n)
    ref = O.OracleParser(17, [bench.ORACLE_DEC[d] for d in cfg["decoders"]], outputs=cfg["outputs"]).decode(
        hd, ho, hc, nthreads=8, layouts=False)
    assert np.array_equal(got["records"], ref["records"].view(np.uint8).reshape(n, 16)[idx])
    assert np.array_equal(got["err_args"], ref["err_args"].reshape(n, 2)[idx])
    want = np.ascontiguousarray(ref["flows"].reshape(3, n)[:, idx].T)
    assert np.array_equal(got["flows"], want.view(np.uint8).reshape(k, 24))
