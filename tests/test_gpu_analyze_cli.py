"""GPU: analyze_distribution.py end to end, as a user runs it: a saved random policy scored on two difficulties with
the same seeds, zero-shot and after one adaptation step; one JSON file with the per-difficulty arrays, their means and
the pairwise distances.  Episodes are capped at 48 steps through the scenario file to keep the run short."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "ppo-2dgrid_amd", "analyze_distribution.py")

YAML = """
global:
  max_steps: 48
difficulties:
  easy:
    env_id: MERLIN-Easy-v0
    params: {render_mode: rgb_array, size: 16}
  hard:
    env_id: MERLIN-Hard-v0
    params: {render_mode: rgb_array, size: 16}
"""


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    from merlin.actor_critic import CNNActorCritic

    d = tmp_path_factory.mktemp("analyze")
    torch.manual_seed(5)
    torch.save(CNNActorCritic((56, 56, 3), 3).state_dict(), d / "policy.pth")
    (d / "scenario.yaml").write_text(YAML)
    return d


@pytest.mark.parametrize("extra", [["--adapt_steps", "0"], ["--adapt_steps", "1", "--k_support", "16"]],
                         ids=["zero_shot", "one_shot"])
def test_cli_writes_the_analysis(saved, extra):
    out = saved / f"out_{extra[1]}.json"
    r = subprocess.run([sys.executable, SCRIPT, "--model_path", str(saved / "policy.pth"), "--difficulties", "easy",
                        "hard", "--num_tasks", "4", "--base_seed", "300000", "--config", str(saved / "scenario.yaml"),
                        "--out", str(out)] + extra, cwd=saved, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert res["difficulties"] == ["easy", "hard"] and res["adapt_steps"] == int(extra[1])
    assert set(res["per_difficulty"]) == {"easy", "hard"}
    for d in ("easy", "hard"):
        p = res["per_difficulty"][d]
        assert len(p["rewards"]) == len(p["steps"]) == len(p["losses"]) == 4
        assert all(1 <= s <= 48 for s in p["steps"])
        assert abs(p["reward_mean"] - sum(p["rewards"]) / 4) <= 1e-12
        for k in ("reward_mean", "reward_std", "steps_mean", "steps_std"):
            assert math.isfinite(p[k]), (d, k)
    assert list(res["pairwise"]) == ["easy|hard"]
    dist = res["pairwise"]["easy|hard"]
    assert set(dist) == {"mean_norm_diff", "kl_ab", "kl_ba", "js_div", "wasserstein"}
    assert all(math.isfinite(v) for v in dist.values()), dist
