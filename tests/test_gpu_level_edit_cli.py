"""GPU: ppo_train.py --level_replay accel --save_levels end to end on a tiny budget: the saved bank loads with its
lineage, some level was edited, and the editing scalars are logged."""
import os

import pytest

pytestmark = pytest.mark.gpu


def _load_cli():
    import importlib.util

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppo-2dgrid_amd", "ppo_train.py")
    spec = importlib.util.spec_from_file_location("ppo_train", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_accel_run_saves_the_evolved_bank(tmp_path, monkeypatch, device):
    from merlin.levels import LevelSet

    mod = _load_cli()
    monkeypatch.chdir(tmp_path)
    logged = {}
    add = mod.ScalarLog.add_scalar

    def record(self, tag, value, step):
        logged.setdefault(tag, []).append(float(value))
        add(self, tag, value, step)

    monkeypatch.setattr(mod.ScalarLog, "add_scalar", record)
    out = tmp_path / "bank.npz"
    args = mod.parse_args(["--device", "cuda", "--difficulty", "mediumhard", "--seed", "777", "--num_envs", "64",
                           "--k_steps", "16", "--minibatch_size", "512", "--update_epochs", "1",
                           "--total_steps", "2048", "--eval_episodes", "1", "--num_levels", "32", "--level_replay",
                           "accel", "--accel_edits", "3", "--save_levels", str(out), "--group_timestamp", "T"])
    assert args.accel_children is None and args.accel_min_dist == 1 and args.accel_every == 1
    agent = mod.train_minigrid(args)
    assert agent.level_editor.children == 4 and agent.level_editor.generation == 2  # L / 8 children, two rounds
    bank = LevelSet.load(str(out))
    assert len(bank) == 32 and bank.size == 16
    assert (bank.generation > 0).any() and ((bank.generation > 0) == (bank.parent >= 0)).all()
    live = agent.level_set
    assert (bank.walls == live.walls.cpu()).all() and (bank.generation == live.generation.cpu()).all()
    for tag in ("levels/children_accepted", "levels/generation_mean", "levels/edited_share",
                "levels/optimal_steps_mean", "levels/train_success", "levels/seen"):
        assert len(logged[tag]) == 2, tag
    assert sum(logged["levels/children_accepted"]) == int(agent.level_editor.accepted.item()) > 0
    assert logged["levels/edited_share"][-1] == float((bank.generation > 0).double().mean())
    assert logged["levels/optimal_steps_mean"][-1] > 0


def test_cli_accel_needs_a_level_set(device):
    mod = _load_cli()
    with pytest.raises(SystemExit):
        mod.train_minigrid(mod.parse_args(["--device", "cuda", "--num_envs", "64", "--level_replay", "accel"]))
