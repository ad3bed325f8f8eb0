"""Optimal path lengths and the path-efficiency metrics built on them.

Raw reward and episode length are confounded by the map: the shortest possible episode of a ``hard`` 32x32 task takes
15 to 60 actions, of a ``medium`` 5x5 task 1 to 6.  ``dist`` -- the least number of actions after which an episode
started in a pose terminates at the goal, turns costing an action each, -1 if none does (include/merlin_hip.h
merlin_shortest_paths) -- comes from one HIP kernel for every env of a vector env (``MerlinVecEnv.optimal_steps`` /
``distance_field``, ``merlin._native.shortest_paths``).  On top of it:

``optimal_reward``       the reward of the episode that takes dist actions: the env's own expression, 0 when the task
                         cannot be solved inside max_steps.
``optimal_paths``        dist and the optimal reward of seed i's start pose, task by task as every ``evaluate_*``
                         function of merlin.evaluation plays them.
``oracle_actions``       a shortest-path action for every pose, read off the distance field.
``path_metrics``         success rate, SPL (success weighted by path length: Anderson et al., "On Evaluation of
                         Embodied Navigation Agents", 2018), excess steps, reward ratio and regret over the solvable
                         tasks.
``evaluate_efficiency``  evaluate, then score against the optimum.
"""
from __future__ import annotations

import numpy as np
import torch

from .evaluation import SWEEP_SEED_BASE, evaluate_few_shot, evaluate_seeds
from .pose_fields import VEC, seeded_env


def optimal_reward(dist, max_steps: int):
    """float32, torch or numpy as `dist`: (float)(1.0 - 0.9 * ((double)dist / (double)max_steps)) where 1 <= dist <=
    max_steps -- the expression of the env's step (MiniGridEnv._reward), so an optimal episode's return equals it bit
    for bit -- and 0 elsewhere.  A task with dist == max_steps is solvable, with reward 0.1."""
    ms = int(max_steps)
    if isinstance(dist, torch.Tensor):
        d = dist.to(torch.float64)
        ok = (dist >= 1) & (dist <= ms)
        return torch.where(ok, 1.0 - 0.9 * (d / float(ms)), torch.zeros((), dtype=torch.float64, device=d.device)).float()
    dist = np.asarray(dist)
    ok = (dist >= 1) & (dist <= ms)
    return np.where(ok, 1.0 - 0.9 * (dist.astype(np.float64) / float(ms)), 0.0).astype(np.float32)


def optimal_paths(seeds, difficulty="mediumhard", size: int = 16, device="cuda", max_steps: int | None = None):
    """(opt_steps list[int], opt_rewards list[float]): dist of the start pose of seed i's task and its optimal reward.
    One seeded vector env (`difficulty`: one name, or one per seed), one reset and one kernel.  Every evaluate_*
    function plays seed i's map from reset(seed=i), so the result lines up with their outputs task by task."""
    seeds = [int(s) for s in seeds]
    if not seeds:
        return [], []
    with seeded_env(seeds, difficulty, size, device, max_steps) as env:
        dist, ms = env.optimal_steps(), env.max_steps
    return dist.cpu().tolist(), optimal_reward(dist, ms).cpu().tolist()


def level_optimal_steps(level_set) -> torch.Tensor:
    """int32[L] on the set's device: dist of every level of a merlin.levels.LevelSet from its start pose, one launch."""
    from . import _native as nat

    return nat.shortest_paths(level_set.walls, level_set.goal, level_set.agent, level_set.size)


def oracle_actions(field: torch.Tensor, walls: torch.Tensor, goal: torch.Tensor, agent: torch.Tensor) -> torch.Tensor:
    """int64[n]: an action on a shortest path for each pose agent[q] = (x, y, dir, 0) of map q -- field int16[n, 4, S,
    S] (MerlinVecEnv.distance_field), walls int32[n, S], goal int32[n, 2] (snapshot()), all on one device.  Forward
    if the front cell is the goal; otherwise the successor of least dist among forward (only if the front cell is
    free), left, right, ties broken in that order; action 0 where the pose's dist is -1."""
    n, _, S, _ = field.shape
    dev = field.device
    q = torch.arange(n, device=dev)
    x, y, d = agent[:, 0].long(), agent[:, 1].long(), agent[:, 2].long() & 3
    vec = torch.tensor(VEC, dtype=torch.int64, device=dev)
    fx, fy = x + vec[d, 0], y + vec[d, 1]
    inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
    fxc, fyc = fx.clamp(0, S - 1), fy.clamp(0, S - 1)
    front_free = inside & (((walls[q, fyc].long() >> fxc) & 1) == 0)
    front_goal = (fx == goal[:, 0].long()) & (fy == goal[:, 1].long())
    big = torch.full((n,), 1 << 20, dtype=torch.int64, device=dev)

    def value(v, ok):  # a successor's dist, "none" as a large number
        v = v.long()
        return torch.where(ok & (v >= 0), v, big)

    xc, yc = x.clamp(0, S - 1), y.clamp(0, S - 1)
    here = torch.where((x == xc) & (y == yc), field[q, d, yc, xc].long(), -torch.ones_like(x))
    cand = torch.stack([value(field[q, d, fyc, fxc], front_free),            # forward
                        value(field[q, (d + 3) & 3, yc, xc], here >= 0),     # left
                        value(field[q, (d + 1) & 3, yc, xc], here >= 0)])    # right
    best = cand.argmin(0)  # the first minimum: forward, left, right
    action = torch.tensor([2, 0, 1], dtype=torch.int64, device=dev)[best]
    action = torch.where(front_goal, torch.full_like(action, 2), action)
    return torch.where(here >= 0, action, torch.zeros_like(action))


def path_metrics(rewards, steps, opt_steps, max_steps: int) -> dict:
    """Path efficiency of one episode per task against the optimum (host arrays of one length).

    success = reward > 0.  That holds for unshaped envs only, where the one non-zero reward is the goal's (>= 0.1); a
    stuck penalty or exploration bonus breaks it (evaluate_efficiency refuses them).  solvable = 1 <= opt <= max_steps.
    Over the solvable tasks: success_rate = mean success; spl = mean of success * opt / max(steps, opt);
    excess_steps_mean = mean of steps - opt over the successes; optimal_reward_mean; reward_ratio = mean of reward /
    optimal reward; regret_mean = mean of optimal reward - reward (rewards rounded to float32, as optimal_reward is,
    so an optimal episode has ratio 1 and regret 0 exactly).  Also n_tasks, n_solvable, and under per_task the
    arrays success, solvable, opt_steps, opt_rewards, spl (0 for unsolvable tasks).  With no solvable task the means
    are nan."""
    # rewards at the float32 the env's step emits them in (an f64 episode return of an unshaped env is that one value)
    rew = np.asarray(rewards, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1)
    st = np.asarray(steps, dtype=np.int64).reshape(-1)
    opt = np.asarray(opt_steps, dtype=np.int64).reshape(-1)
    if not (rew.shape == st.shape == opt.shape):
        raise ValueError(f"path_metrics: {rew.size} rewards, {st.size} steps, {opt.size} optimal steps")
    ms = int(max_steps)
    success = rew > 0
    solvable = (opt >= 1) & (opt <= ms)
    opt_rew = optimal_reward(opt, ms).astype(np.float64)
    spl = np.where(solvable & success, opt / np.maximum(np.maximum(st, opt), 1), 0.0)
    sel = solvable
    won = solvable & success

    def mean(v, m):
        return float(np.mean(v[m])) if m.any() else float("nan")

    safe = np.where(sel, opt_rew, 1.0)
    return {
        "n_tasks": int(rew.size),
        "n_solvable": int(sel.sum()),
        "success_rate": mean(success.astype(np.float64), sel),
        "spl": mean(spl, sel),
        "excess_steps_mean": mean((st - opt).astype(np.float64), won),
        "optimal_reward_mean": mean(opt_rew, sel),
        "reward_ratio": mean(rew / safe, sel),
        "regret_mean": mean(opt_rew - rew, sel),
        "per_task": {"success": success, "solvable": solvable, "opt_steps": opt, "opt_rewards": opt_rew, "spl": spl,
                     "rewards": rew, "steps": st},
    }


def evaluate_efficiency(ac, seeds, adapt_steps: int = 0, difficulty="mediumhard", size: int = 16, device="cuda",
                        max_steps: int | None = None, **kw) -> dict:
    """path_metrics of policy `ac` on one task per seed: its deterministic episodes (evaluate_seeds; adapt_steps > 0:
    evaluate_few_shot with lr_inner / k_support / task_batch from kw, as evaluate_across_difficulties chooses), then
    optimal_paths on the same seeds.  Shaped rewards (stuck_penalty, exploration_bonus) are refused: success is read
    off the reward's sign."""
    for flag in ("stuck_penalty", "exploration_bonus"):
        if kw.get(flag):
            raise ValueError(f"evaluate_efficiency: {flag} shapes the reward, and success is defined as reward > 0")
    seeds = [int(s) for s in seeds]
    common = dict(difficulty=difficulty, size=size, device=device, max_steps=max_steps)
    if int(adapt_steps) > 0:
        rew, steps, _ = evaluate_few_shot(ac, seeds, int(adapt_steps), **common, **kw)
    else:
        for k in ("lr_inner", "k_support", "task_batch"):  # few-shot only
            kw.pop(k, None)
        rew, steps = evaluate_seeds(ac, seeds, **common, **kw)
    opt, _ = optimal_paths(seeds, **common)
    ms = int(max_steps) if max_steps else 4 * int(size) * int(size)
    return path_metrics(rew, steps, opt, ms)


def sweep_checkpoints_efficiency(model_dir: str, difficulty: str = "mediumhard", tasks: int = 50, size: int = 16,
                                 device="cuda", max_steps: int | None = None):
    """merlin.evaluation.sweep_checkpoints with the path metrics beside it: [(path, mean reward, mean steps,
    path_metrics dict)] of every *.pth in model_dir on the sweep's fixed seeds, best mean reward first -- the same
    ranking.  The optimum is computed once per sweep, not per checkpoint."""
    import glob
    import os

    from .checkpoints import load_policy

    seeds = range(SWEEP_SEED_BASE, SWEEP_SEED_BASE + tasks)
    common = dict(difficulty=difficulty, size=size, device=device, max_steps=max_steps)
    paths = sorted(glob.glob(os.path.join(model_dir, "*.pth")))
    if not paths:
        return []
    opt, _ = optimal_paths(seeds, **common)
    ms = int(max_steps) if max_steps else 4 * int(size) * int(size)
    results = []
    for path in paths:
        rew, st = evaluate_seeds(load_policy(path, device), seeds, **common)
        results.append((path, sum(rew) / len(rew), sum(st) / len(st), path_metrics(rew, st, opt, ms)))
    results.sort(key=lambda r: r[1], reverse=True)
    return results
