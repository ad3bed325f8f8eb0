"""Generate tests/golden/task_metrics_ref.npz and tests/golden/fewshot_ref.npz from the reference.

Run where the reference checkout exists (make_golden.py's REF), never by a test:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fewshot_golden.py

  task_metrics_ref.npz  the REFERENCE src/metrics/task_metrics.py compare_two_feature_sets on two random feature
                  sets (40, 3) / (25, 3), a 1-D pair and a pair with one constant column (the std floor).
  fewshot_ref.npz the REFERENCE evaluate_few_shot (src/distribution_over_tasks.py:132-209), imported read-only and
                  driven on CPU over a gym-style stub env around oracle/minigrid_literal.LiteralEnv (frames from
                  oracle.render of its view codes; reset(seed=s) always gives seed s's map; max_steps 16, so every
                  24-step support rollout holds a truncation and a reseeded reset): 3 tasks, adapt_steps 2,
                  k_support 24, lr_inner 0.01, torch.manual_seed(0) initial CNNActorCritic weights.  Recorded by
                  wrappers around the env and the fast policy's act (defined here; nothing of the reference is
                  edited): per task and adapt step the rollout (codes, act, rew, val, logp, done, last_val); after
                  adaptation per tensor (norm, sum) and 256 sampled elements of adapted - meta; the final
                  deterministic episode's actions, reward, steps, loss and smallest top-2 logit margin.  Task seeds
                  are taken, in order, from those whose margin is >= 1e-4 at every step of that episode (ten times
                  the 1e-5 to which the batched path reproduces logits), so an argmax flip cannot be rounding.
Only the reference's outputs are stored, arrays and key names.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
from make_golden import REF, _param_checksums  # noqa: E402
from minigrid_literal import LiteralEnv  # noqa: E402
from tiles import build_atlas  # noqa: E402

G, ADAPT_STEPS, K_SUPPORT, LR_INNER, MAX_STEPS = 3, 2, 24, 0.01, 16
MIN_MARGIN = 1e-4


def _import_reference():
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    os.environ["MPLBACKEND"] = "Agg"
    sys.dont_write_bytecode = True
    # the reference's env factory needs gymnasium / minigrid, which this generator replaces with the stub env below
    pkg = types.ModuleType("src.scenario_creator")
    pkg.__path__ = []
    mod = types.ModuleType("src.scenario_creator.scenario_creator")
    mod.ScenarioCreator = type("ScenarioCreator", (), {})
    pkg.scenario_creator = mod
    sys.modules["src.scenario_creator"] = pkg
    sys.modules["src.scenario_creator.scenario_creator"] = mod
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import src.distribution_over_tasks as dot
    from src.actor_critic import CNNActorCritic
    from src.metrics import task_metrics

    return dot, CNNActorCritic, task_metrics


def gen_task_metrics(task_metrics):
    rs = np.random.RandomState(17)
    const = rs.randn(30, 2)
    const[:, 1] = 0.75  # a constant column: std = the 1e-8 floor
    cases = {"a": (rs.randn(40, 3), 0.5 + 1.5 * rs.randn(25, 3)),
             "b": (rs.rand(31), rs.rand(18) ** 2),
             "c": (const, const + np.array([0.25, 0.0]))}
    keys = ("mean_norm_diff", "kl_ab", "kl_ba", "js_div", "wasserstein")
    rec = {"keys": np.array(keys)}
    for name, (x, y) in cases.items():
        out = task_metrics.compare_two_feature_sets(x, y)
        rec[f"{name}_x"], rec[f"{name}_y"] = x, y
        rec[f"{name}_out"] = np.array([out[k] for k in keys], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "task_metrics_ref.npz"), **rec)


class _StubEnv:
    """gym-style env over LiteralEnv that logs what the reference's loops see."""

    def __init__(self, atlas):
        self.atlas = atlas
        self.env = LiteralEnv(16, "mediumhard", max_steps=MAX_STEPS)
        self.codes = None  # view codes of the current observation
        self.steps = []  # (reward, done) per step

    def _obs(self, codes):
        self.codes = np.asarray(codes, dtype=np.uint8).reshape(49)
        return O.render(self.codes[None], self.atlas)[0]

    def reset(self, seed=None):
        return self._obs(self.env.reset(seed)), {}

    def step(self, action):
        codes, r, term, trunc = self.env.step(int(action))
        self.steps.append((float(r), bool(term or trunc)))
        return self._obs(codes), r, bool(term), bool(trunc), {}


def _run_task(dot, CNNActorCritic, meta, atlas, seed):
    import torch

    env = _StubEnv(atlas)
    fast = CNNActorCritic((56, 56, 3), 3)
    calls = []  # (codes, deterministic, action, logp, value, top-2 logit margin) per fast.act call
    act_orig = fast.act

    def act_wrap(obs, deterministic=False):
        a, lp, v = act_orig(obs, deterministic=deterministic)
        with torch.no_grad():
            logits = fast.actor(fast.actor_extractor(fast._format_obs(obs)))
            top = torch.topk(logits[0], 2).values
        calls.append((env.codes.copy(), bool(deterministic), int(a.item()), float(lp.item()), float(v.item()),
                      float(top[0] - top[1])))
        return a, lp, v

    fast.act = act_wrap
    torch.manual_seed(1000 + seed)  # the support rollouts' draws (recorded, so only this generator depends on it)
    reward, steps, loss = dot.evaluate_few_shot(env, fast, meta, seed, True, torch.device("cpu"), LR_INNER, K_SUPPORT,
                                                ADAPT_STEPS)
    rec = {}
    per = K_SUPPORT + 1  # k acting calls + the bootstrap value's call per adapt step
    for s in range(ADAPT_STEPS):
        cs, st = calls[s * per:(s + 1) * per], env.steps[s * K_SUPPORT:(s + 1) * K_SUPPORT]
        assert not any(c[1] for c in cs) and any(d for _, d in st)
        rec[f"a{s}_codes"] = np.stack([c[0] for c in cs])  # [k + 1, 49]
        rec[f"a{s}_act"] = np.array([c[2] for c in cs[:-1]], dtype=np.int64)
        rec[f"a{s}_logp"] = np.array([c[3] for c in cs[:-1]], dtype=np.float32)
        rec[f"a{s}_val"] = np.array([c[4] for c in cs[:-1]], dtype=np.float32)
        rec[f"a{s}_last_val"] = np.float32(cs[-1][4])
        rec[f"a{s}_rew"] = np.array([r for r, _ in st], dtype=np.float32)
        rec[f"a{s}_done"] = np.array([d for _, d in st], dtype=np.float32)
    ep = calls[ADAPT_STEPS * per:]
    assert len(ep) == steps + 1 and all(c[1] for c in ep[:-1])
    rec["ep_actions"] = np.array([c[2] for c in ep[:-1]], dtype=np.int64)
    rec["ep_reward"], rec["ep_steps"], rec["ep_loss"] = np.float64(reward), np.int64(steps), np.float64(loss)
    rec["ep_margin"] = np.float64(min(c[5] for c in ep[:-1]))
    delta = {n: (p.detach() - q.detach()).reshape(-1).double() for (n, p), (_, q) in
             zip(fast.named_parameters(), meta.named_parameters())}
    return rec, delta


def gen_fewshot(dot, CNNActorCritic):
    import torch

    atlas = build_atlas()
    torch.manual_seed(0)
    meta = CNNActorCritic((56, 56, 3), 3)
    keys, sums0 = _param_checksums(meta)
    names = [n for n, _ in meta.named_parameters()]
    rec = {"cfg": np.array([G, ADAPT_STEPS, K_SUPPORT, MAX_STEPS], dtype=np.int64), "lr_inner": np.float64(LR_INNER),
           "keys": keys, "sums0": sums0, "names": np.array(names)}
    seeds, seed = [], 100000
    while len(seeds) < G:
        task, delta = _run_task(dot, CNNActorCritic, meta, atlas, seed)
        if float(task["ep_margin"]) >= MIN_MARGIN:
            g = len(seeds)
            seeds.append(seed)
            for k, v in task.items():
                rec[f"t{g}_{k}"] = v
            stats, idx, vals = [], [], []
            for i, n in enumerate(names):
                d = delta[n]
                stats.append([d.norm().item(), d.sum().item()])
                sel = np.sort(np.random.RandomState(i + 1).choice(d.numel(), min(256, d.numel()), replace=False))
                idx.append(np.pad(sel, (0, 256 - sel.size), constant_values=-1))
                vals.append(np.pad(d.numpy()[sel], (0, 256 - sel.size)))
            rec[f"t{g}_delta_stats"] = np.array(stats)
            rec[f"t{g}_delta_idx"] = np.array(idx, dtype=np.int64)
            rec[f"t{g}_delta_vals"] = np.array(vals)
        seed += 1
        assert seed < 100100, "no task seeds with a clear argmax margin"
    rec["seeds"] = np.array(seeds, dtype=np.int64)
    assert all(float(rec[f"t{g}_ep_margin"]) >= MIN_MARGIN for g in range(G))
    np.savez_compressed(os.path.join(HERE, "fewshot_ref.npz"), **rec)
    for g in range(G):
        print(f"task {seeds[g]}: steps {int(rec[f't{g}_ep_steps'])} reward {float(rec[f't{g}_ep_reward']):.4f} "
              f"loss {float(rec[f't{g}_ep_loss']):.6f} margin {float(rec[f't{g}_ep_margin']):.2e}")


if __name__ == "__main__":
    dot, CNNActorCritic, task_metrics = _import_reference()
    gen_task_metrics(task_metrics)
    gen_fewshot(dot, CNNActorCritic)
    print("few-shot fixtures written to", HERE)
