"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run as a fresh child process at a small shape: one JSON line
with the headline fields, K timed steps, nothing of what --full adds (tiers, CPU baseline, the GEMMs timed alone),
and --dump-outputs writing the last timed step's arrays as float .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 256, 16


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--num-envs", str(N), "--k-steps", str(T), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-4000:]
    out = json.loads(lines[0])
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "fp32"
    assert out["metric"].startswith("env-steps/sec") and out["n_gpus"] == 1
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    # value = the timed steps' env-steps over their time
    assert abs(out["value"] - N * T / (out["ms_per_step"] / 1e3)) / out["value"] < 0.01
    for k in ("tiers", "cpu_baseline", "roofline_x6_standalone"):
        assert k not in out, k
    assert out["kernels"] and out["phases_ms"]["update"] > 0  # read from the timed steps' own events

    names = sorted(f[:-4] for f in os.listdir(out_dir))
    assert names == sorted(["last_value", "update_stats", "actions", "logprobs", "values", "rewards", "dones",
                            "advantages", "returns", "parameters"])
    arrays = {n: np.load(out_dir / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["last_value"].shape == (N,) and arrays["update_stats"].shape == (6,)
    for n in ("actions", "logprobs", "values", "rewards", "dones", "advantages", "returns"):
        assert arrays[n].shape == (T, N), n
    assert set(np.unique(arrays["actions"])) <= {0.0, 1.0, 2.0} and set(np.unique(arrays["dones"])) <= {0.0, 1.0}
    assert arrays["parameters"].ndim == 1 and arrays["parameters"].size > 500_000
