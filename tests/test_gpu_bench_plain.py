"""A plain bench.py run (no --full) on the GPU at a small size: only the headline path is timed, --steps sets the
number of timed steps, the line carries the contract keys with ms_per_step, and --dump-outputs writes the last
step's accept bytes as float32, equal to the decisions the seeded inputs were constructed for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_line_and_dumped_outputs(tmp_path):
    import bench
    n, steps = 8800, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--shares", str(n), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    head = json.loads(lines[-1])
    assert head["steps"] == steps and head["warmup"] == 1 and head["n_gpus"] == 1
    assert head["unit"] == "share verifications/s" and head["higher_is_better"] is True
    assert head["dtype"].startswith("u32") and head["config"]["decision_mismatches"] == 0
    assert head["ms_per_step"] > 0
    assert abs(head["value"] - n / (head["ms_per_step"] * 1e-3)) <= 1e-4 * head["value"]
    detail = json.loads([x for x in lines if x.startswith("BENCH_DETAIL ")][-1][len("BENCH_DETAIL "):])
    assert detail["tpke_batched"]["pipeline"] == 4 and detail["tpke_batched"]["steps"] == steps
    for leg in ("tpke_exact", "tpke_byzantine", "msm", "threshold_signature", "epoch_replay", "ecdsa_headers", "dkg",
                "rbc_erasure_coding", "mcl_latency", "cpu_baseline"):
        assert detail[leg] is None, leg
    assert "single_batch" not in detail["tpke_batched"]
    assert os.listdir(tmp_path / "out") == ["accept.npy"]
    acc = np.load(tmp_path / "out" / "accept.npy")
    assert acc.dtype == np.float32 and acc.shape == (n,)
    expect = np.ones(n, dtype=np.float32)       # bench.make_inputs: 1 % of the shares corrupted at seeded positions
    expect[np.random.default_rng(bench.SEED).choice(n, size=round(0.01 * n), replace=False)] = 0
    assert np.array_equal(acc, expect)
