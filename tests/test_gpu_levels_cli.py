"""GPU: ppo_train.py on a finite level set, end to end at a tiny budget: --num_levels with prioritized replay writes
the levels/* scalars and the checkpoints, and --level_file trains on a saved set."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LEVEL_TAGS = {"levels/train_success", "levels/test_success", "levels/gap", "levels/train_return",
              "levels/test_return", "levels/return_gap", "levels/seen", "levels/score_mean"}


def _load_cli():
    import importlib.util

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppo-2dgrid_amd", "ppo_train.py")
    spec = importlib.util.spec_from_file_location("ppo_train", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _scalars(tb_dir):
    """{tag: [values]} and the histogram tags of a run's log: the JSONL stand-in, or TensorBoard's event files."""
    path = os.path.join(tb_dir, "scalars.jsonl")
    vals, hists = {}, set()
    if os.path.exists(path):
        for ln in open(path):
            row = json.loads(ln)
            if "value" in row:
                vals.setdefault(row["tag"], []).append(row["value"])
            elif "histogram" in row:
                hists.add(row["tag"])
        return vals, hists
    from tensorboard.backend.event_processing.event_accumulator import EventAccumulator

    acc = EventAccumulator(tb_dir)
    acc.Reload()
    for tag in acc.Tags()["scalars"]:
        vals[tag] = [e.value for e in acc.Scalars(tag)]
    return vals, set(acc.Tags()["histograms"])


COMMON = ["--device", "cuda", "--difficulty", "mediumhard", "--seed", "777", "--num_envs", "64", "--k_steps", "8",
          "--minibatch_size", "256", "--update_epochs", "1", "--total_steps", "1024", "--eval_episodes", "4"]


def test_cli_num_levels_plr(tmp_path, monkeypatch, device):
    mod = _load_cli()
    monkeypatch.chdir(tmp_path)
    agent = mod.train_minigrid(mod.parse_args(COMMON + ["--num_levels", "8", "--level_seed_base", "50",
                                                        "--level_replay", "plr", "--group_timestamp", "LV"]))
    assert len(agent.level_set) == 8 and agent.level_set.seeds == list(range(50, 58))
    assert agent.level_sampler.strategy == "plr" and agent.level_iteration == 2  # 2 x 512 steps
    d = tmp_path / "checkpoints" / "MERLIN-MediumHard-v0_16x16_mediumhard_LV" / "seed_777"
    assert {"best_model.pth", "ppo_model_final.pth", "ppo_model_1k.pth"} <= set(os.listdir(d))
    sd = torch.load(d / "ppo_model_final.pth", weights_only=True)
    assert set(sd) == set(agent.ac.state_dict())
    vals, hists = _scalars(str(tmp_path / "tb_logs" / "MERLIN-MediumHard-v0_16x16_mediumhard_LV" / "seed_777"))
    assert LEVEL_TAGS <= set(vals) and "levels/sampling_weights" in hists
    for tag in LEVEL_TAGS:
        assert len(vals[tag]) == 2 and np.isfinite(vals[tag]).all(), tag
    assert all(1 <= v <= 8 for v in vals["levels/seen"])
    for a, b, g in zip(vals["levels/train_success"], vals["levels/test_success"], vals["levels/gap"]):
        assert 0 <= a <= 1 and 0 <= b <= 1 and abs(g - (a - b)) < 1e-6


def test_cli_level_file_round_trip(tmp_path, monkeypatch, device):
    from merlin.levels import LevelSet

    mod = _load_cli()
    monkeypatch.chdir(tmp_path)
    ls = LevelSet.from_seeds(range(90, 96), difficulties=["medium", "mediumhard"] * 3, size=16, device=device)
    ls.save(str(tmp_path / "six.npz"))
    agent = mod.train_minigrid(mod.parse_args(COMMON + ["--level_file", str(tmp_path / "six.npz"),
                                                        "--group_timestamp", "LF"]))
    got = agent.level_set
    assert len(got) == 6 and got.seeds == list(range(90, 96)) and got.difficulties == ["medium", "mediumhard"] * 3
    for f in ("walls", "goal", "agent"):
        assert torch.equal(getattr(got, f), getattr(ls, f))
    assert agent.level_sampler.strategy == "uniform"
    lv = agent.buf.levels.cpu().numpy()
    assert lv.min() >= 0 and lv.max() < 6
    vals, _ = _scalars(str(tmp_path / "tb_logs" / "MERLIN-MediumHard-v0_16x16_mediumhard_LF" / "seed_777"))
    assert LEVEL_TAGS <= set(vals)
