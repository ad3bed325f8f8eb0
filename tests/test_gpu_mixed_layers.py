"""GPU: per-env difficulties through the layers above the env -- evaluation (per-seed difficulty lists, the
cross-difficulty pass), PPO's per-difficulty episode statistics, FOMAML's per-task difficulties under replayed
graphs, few-shot evaluation.  Episodes are checked by replaying their recorded actions through the C oracle with each
env's own class, as tests/test_gpu_eval.py::test_eval_matches_oracle_replay does for one difficulty."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ["easy", "medium", "mediumhard", "hard", "hardest"]
MAX_STEPS = 48


@pytest.fixture(scope="module")
def policy(device):
    from merlin.actor_critic import CNNActorCritic

    torch.manual_seed(7)
    return CNNActorCritic((56, 56, 3), 3).to(device)


def assert_oracle_replay(oracle, seeds, names, acts, rew, steps, size=16, max_steps=MAX_STEPS):
    """Rewards (f64 sum of the oracle's rewards up to the first done) and steps of recorded episodes, class by class."""
    seeds = np.asarray(seeds, dtype=np.uint64)
    names = np.asarray(names)
    acts = np.asarray(acts)
    for d in sorted(set(names)):
        idx = np.flatnonzero(names == d)
        _, orew, oterm, otrunc, _ = oracle.batch_rollout(seeds[idx], np.ascontiguousarray(acts[:, idx]), size=size,
                                                         difficulty=str(d), max_steps=max_steps)
        done = np.maximum(oterm, otrunc).astype(bool)
        for j, i in enumerate(idx):
            assert done[:, j].any(), (d, i)  # every episode ended inside the recorded actions
            first = int(np.argmax(done[:, j]))
            assert steps[i] == first + 1, (d, i, steps[i], first + 1)
            assert abs(rew[i] - float(orew[: first + 1, j].astype(np.float64).sum())) <= 1e-6, (d, i)


def test_evaluate_seeds_per_seed_difficulties(oracle, device, policy):
    from merlin.evaluation import evaluate_seeds

    names = [d for d in NAMES for _ in range(4)]
    seeds = list(range(2500, 2500 + len(names)))
    rew, steps, acts = evaluate_seeds(policy, seeds, difficulty=names, size=16, device=device, max_steps=MAX_STEPS,
                                      record=True)
    assert len(rew) == len(steps) == 20
    assert_oracle_replay(oracle, seeds, names, acts.numpy(), rew, steps)
    with pytest.raises(ValueError):
        evaluate_seeds(policy, seeds, difficulty=names[:-1], device=device)


def test_evaluate_across_difficulties(oracle, device, policy):
    """One entry per name, num_tasks long, every difficulty on the same seeds; the entry of d equals
    evaluate_seeds(difficulty=[d] * num_tasks) on those seeds, itself replayed through the oracle."""
    from merlin.evaluation import evaluate_across_difficulties, evaluate_seeds

    num_tasks, base = 4, 300000
    res = evaluate_across_difficulties(policy, NAMES, num_tasks=num_tasks, base_seed=base, device=device,
                                       max_steps=MAX_STEPS)
    assert list(res) == NAMES
    seeds = [base + i for i in range(num_tasks)]
    for d in NAMES:
        rew, steps, losses = res[d]
        assert len(rew) == len(steps) == len(losses) == num_tasks and all(math.isfinite(x) for x in losses)
        r2, s2, acts = evaluate_seeds(policy, seeds, difficulty=[d] * num_tasks, device=device, max_steps=MAX_STEPS,
                                      record=True)
        assert rew == r2 and steps == s2, d
        assert_oracle_replay(oracle, seeds, [d] * num_tasks, acts.numpy(), rew, steps)
    with pytest.raises(ValueError):
        evaluate_across_difficulties(policy, ["easy", "easy"], num_tasks=2, device=device)


def test_ppo_episode_stats_by_difficulty(device):
    """The kernel's per-difficulty statistics of a mixed rollout against the same sums on the host, under the bound
    of tests/test_gpu_episode_stats.py (count * 2^-53 * sum|x| against math.fsum); then one update."""
    from merlin import MerlinVecEnv
    from merlin import _native as nat
    from merlin.ppo import PPO
    from merlin.task_mix import assign

    n, k = 256, 16
    names = assign(n, {"easy": 1, "hard": 1})
    assert names == ["easy"] * 128 + ["hard"] * 128
    env = MerlinVecEnv(n, difficulty=names, size=16, seed=99, device=device, max_steps=12)
    torch.manual_seed(0)
    agent = PPO(env, batch_size=n * k, minibatch_size=n * 4, update_epochs=1, device=device)
    last_value = agent.collect_rollouts()
    buf = agent.buf
    done = buf.dones.cpu().numpy() != 0
    ret, length = buf.ep_return.cpu().numpy(), buf.ep_length.cpu().numpy()
    cls = env.class_ids.cpu().numpy()
    raw = agent.episode_class_stats().cpu().numpy()
    got = agent.episode_stats_by_difficulty()
    assert list(got) == ["easy", "hard"]
    u = 2.0 ** -53
    for d in NAMES:
        c = nat.DIFFICULTY_IDS[d]
        m = done & (cls == c)[None, :]
        x = ret[m]
        cnt = int(m.sum())
        assert raw[c, 0] == cnt and raw[c, 3] == int(length[m].sum()), d
        assert abs(raw[c, 1] - math.fsum(x)) <= cnt * u * math.fsum(np.abs(x)), d
        assert abs(raw[c, 2] - math.fsum(x * x)) <= cnt * u * math.fsum(x * x), d
        if d in got:
            assert cnt >= 128  # max_steps 12 in 16 steps: every env finished an episode
            e, mean, std, mlen = got[d]
            assert e == cnt
            assert abs(mean - x.mean()) <= 1e-12 and abs(std - x.std()) <= 1e-9 and abs(mlen - length[m].mean()) <= 1e-9
        else:
            assert cnt == 0 and (raw[c] == 0).all()
    stats = agent.update(last_value)
    assert all(np.isfinite(v) for v in stats.values()), stats
    env.close()


def _assert_task_maps(oracle, env, names, seeds, size=16):
    """In reseed mode the walls and the goal of every task env are its seed's map of its class at any time."""
    st = env.get_state()
    for g, (d, s) in enumerate(zip(names, seeds)):
        cells, meta = oracle.gen_map(size, d, int(s))
        assert ((st["cells"][g] == 1) == (cells == 1)).all(), (g, d)
        assert tuple(st["goal_pos"][g]) == tuple(meta[3:5]), (g, d)


def test_fomaml_task_difficulties_under_replayed_graphs(oracle, device):
    """CAPTURE_AFTER + 2 meta steps on one object, the tasks' classes (and seeds) changing every step: the replayed
    rollout graphs read the new classes from the env's class buffer -- the task envs hold gen_map(size, diff_g,
    seed_g) after each step -- and nothing fell back to eager launches.  Then None: every task back on the object's
    own difficulty, still through the same graphs."""
    from merlin import ScenarioCreator
    from merlin import fomaml as F

    torch.manual_seed(1)
    fm = F.FOMAML(ScenarioCreator(), device=device, difficulty="mediumhard")
    G, k = 8, 16
    graphs = None
    for step in range(F.CAPTURE_AFTER + 2):
        names = [NAMES[(g + step) % 5] for g in range(G)]
        seeds = [7000 + 10 * step + g for g in range(G)]
        out = fm.meta_train_step(seeds, k_support=k, k_query=k, task_difficulties=names)
        assert math.isfinite(out[0])
        assert fm._env.difficulties == names
        _assert_task_maps(oracle, fm._env, names, seeds)
        now = (fm._rollouts["support"]["graph"], fm._rollouts["query"]["graph"])
        assert now[0] is not None and now[1] is not None
        assert graphs is None or (now[0] is graphs[0] and now[1] is graphs[1])  # captured once, then replayed
        graphs = now
    assert fm.capture_steps is True and fm.rollout_graph is True
    st = fm._steps[(G, k, k)]
    assert st.get("inner") is not None and st.get("outer") is not None
    seeds = [9000 + g for g in range(G)]
    fm.meta_train_step(seeds, k_support=k, k_query=k)
    _assert_task_maps(oracle, fm._env, ["mediumhard"] * G, seeds)
    assert fm._rollouts["support"]["graph"] is graphs[0]
    fm._env.errors()


def test_fomaml_first_uniform_then_per_task(oracle, device):
    """A rollout graph captured while the task env was uniform reads no class buffer: the first per-task assignment
    drops it, so the classes still take effect."""
    from merlin import ScenarioCreator
    from merlin.fomaml import FOMAML

    torch.manual_seed(2)
    fm = FOMAML(ScenarioCreator(), device=device, difficulty="medium")
    G, k = 4, 8
    seeds = [41, 42, 43, 44]
    fm.meta_train_step(seeds, k_support=k, k_query=k)
    _assert_task_maps(oracle, fm._env, ["medium"] * G, seeds)
    g0 = fm._rollouts["support"]["graph"]
    names = ["hard", "easy", "hardest", "mediumhard"]
    fm.meta_train_step(seeds, k_support=k, k_query=k, task_difficulties=names)
    _assert_task_maps(oracle, fm._env, names, seeds)
    assert fm._rollouts["support"]["graph"] is not g0


def test_few_shot_zero_steps_equals_zero_shot(device, policy):
    """adapt_steps = 0 with a per-seed class list: the rewards and steps of evaluate_zero_shot with that list (10
    seeds 8 at a time: the last chunk is padded by its last seed and that seed's class)."""
    from merlin.evaluation import evaluate_few_shot, evaluate_zero_shot

    names = [NAMES[i % 5] for i in range(10)]
    seeds = list(range(8100, 8110))
    r0, s0, _ = evaluate_zero_shot(policy, seeds, difficulty=names, device=device, max_steps=MAX_STEPS)
    r1, s1, l1 = evaluate_few_shot(policy, seeds, 0, difficulty=names, device=device, max_steps=MAX_STEPS,
                                   task_batch=8)
    assert r1 == r0 and s1 == s0 and len(l1) == 10
    with pytest.raises(ValueError):
        evaluate_few_shot(policy, seeds, 0, difficulty=names[:3], device=device)


def test_ppo_train_cli_difficulty_mix(tmp_path, monkeypatch, capsys, device):
    """ppo_train.py --difficulty_mix at a tiny budget: the vector env is split among the difficulties, every
    iteration prints the per-difficulty line and logs train_by_difficulty/<name>/ scalars; evaluation and the run's
    name still follow --difficulty."""
    import importlib.util
    import json
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppo-2dgrid_amd", "ppo_train.py")
    spec = importlib.util.spec_from_file_location("ppo_train_mix", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.chdir(tmp_path)
    logged = []
    real = mod.ScalarLog.add_scalar

    def spy(self, tag, value, step):
        logged.append((tag, float(value), int(step)))
        return real(self, tag, value, step)

    monkeypatch.setattr(mod.ScalarLog, "add_scalar", spy)
    args = mod.parse_args(["--device", "cuda", "--difficulty", "easy", "--difficulty_mix", "easy:1,hard:1", "--seed",
                           "5", "--num_envs", "128", "--k_steps", "16", "--minibatch_size", "512", "--update_epochs",
                           "1", "--total_steps", "4096", "--eval_episodes", "1", "--group_timestamp", "MIX"])
    agent = mod.train_minigrid(args)
    assert agent.vec.difficulty == "mixed"
    assert agent.vec.difficulties == ["easy"] * 64 + ["hard"] * 64
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "by difficulty |" in ln]
    assert len(lines) == 2, out[-2000:]  # 2 iterations of 128 x 16 steps
    assert re.search(r"easy: (R -?[\d.]+ len [\d.]+ \(\d+ ep\)|no episode) \| hard: ", lines[0]), lines[0]
    tags = {t for t, _, _ in logged}
    assert {"train_by_difficulty/easy/episodes", "train_by_difficulty/hard/episodes"} <= tags
    assert (tmp_path / "checkpoints" / "MERLIN-Easy-v0_16x16_easy_MIX" / "seed_5" / "ppo_model_final.pth").exists()
    with pytest.raises(SystemExit):
        mod.train_minigrid(mod.parse_args(["--device", "cuda", "--difficulty_mix", "easy:1,hard:1"]))  # one env
