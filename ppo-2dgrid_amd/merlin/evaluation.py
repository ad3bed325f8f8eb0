"""Batched deterministic evaluation and the checkpoint sweep.

``evaluate_policy``  ppo/ppo_train.py:43-69 of the reference: episode ep is reset with
                     ``seed = base_seed + ep`` and run to termination/truncation with the argmax
                     policy.  Here all episodes run at once in one ``MerlinVecEnv`` (env ep seeded
                     base_seed + ep: the same maps), one batched deterministic forward per step, no
                     auto-reset; an env's result is frozen at its first done.  Episode returns are
                     the env's f64 accumulator (the reference sums Python floats), not a sum of the
                     f32 reward buffer.
``evaluate_seeds``   the same for an arbitrary list of seeds (src/sweep_checkpoints.py:52-70
                     evaluate_model: one episode per seed, returns the mean reward and steps).
``sweep_checkpoints`` src/sweep_checkpoints.py:72-100: every ``*.pth`` of a directory on the fixed
                     seeds 200000 + i, ranked by mean reward; checkpoints load through
                     merlin.checkpoints.load_policy (legacy-key remap included).
``evaluate_levels``  the deterministic episode from every level's start pose of a merlin.levels.LevelSet, read off the
                     policy field of the set's maps (one batched forward over their free poses, no stepping); equals
                     evaluate_seeds on a seed-built set.
``evaluate_zero_shot`` src/distribution_over_tasks.py:71-120 for many seeds at once: the
                     deterministic episode's reward and length, and its PPO-style loss -- GAE
                     (gamma .995, lambda .95) over the episode with the value after the last step
                     masked out, advantages normalised over the episode (zeros for a 1-step
                     episode), returns = values + advantages, then -mean(logp) + 0.5 * mean((v -
                     return)^2) with the episode's observations re-evaluated.
``evaluate_few_shot`` src/distribution_over_tasks.py:132-209 for many seeds, a chunk of tasks at a time: per-task
                     adaptation on sampled support rollouts, then the scored deterministic episode
                     (merlin/few_shot.py).
"""
from __future__ import annotations

import glob
import os

import torch

from .envs import MerlinVecEnv

SWEEP_SEED_BASE = 200000  # src/sweep_checkpoints.py:79


def _per_seed(difficulty, n: int):
    """`difficulty` as the env takes it: the name, or the per-seed names as a list of n."""
    if isinstance(difficulty, str):
        return difficulty
    names = [str(d) for d in difficulty]
    if len(names) != n:
        raise ValueError(f"difficulty: {len(names)} names for {n} seeds")
    return names


@torch.no_grad()
def evaluate_seeds(ac, seeds, difficulty="mediumhard", size: int = 16, device="cuda",
                   max_steps: int | None = None, record: bool = False, **env_flags):
    """One deterministic episode per seed, all at once -> (rewards list[float], steps list[int])
    [+ actions int64[T, n] when record: the actions taken, for replay checks].  `difficulty`: one name, or one name
    per seed (a mixed-task vector env: seed i's map comes from difficulty[i]'s generator)."""
    from .actor_critic import MLPActorCritic

    seeds = [int(s) for s in seeds]
    n = len(seeds)
    env = MerlinVecEnv(n, difficulty=_per_seed(difficulty, n), size=size, device=device, max_steps=max_steps, seeds=seeds,
                       **env_flags)
    # an MLP policy (observation.flatten) takes the flattened view its input width names: the RGB partial view
    # (9,408) or the encoded full grid (size * size * 3, observation.fully_observable)
    mlp = isinstance(ac, MLPActorCritic)
    full = mlp and ac.actor[0].in_features == size * size * 3

    def act(obs):
        if not mlp:
            return ac.act_codes(obs, deterministic=True)
        x = env.render_full().reshape(n, -1).float() if full else env.flat_obs(obs)
        return ac.act(x, deterministic=True)

    try:
        obs = env.reset().clone()
        total = torch.zeros(n, dtype=torch.float64, device=env.device)
        steps = torch.zeros(n, dtype=torch.int64, device=env.device)
        done = torch.zeros(n, dtype=torch.bool, device=env.device)
        acts = []
        for _ in range(env.max_steps):
            action, _, _ = act(obs)
            obs, _, term, trunc, info = env.step(action, autoreset=False)
            if record:
                acts.append(action.clone())
            live = ~done
            fin = live & (term | trunc)
            total = torch.where(fin, info["episode_return"], total)
            steps += live.long()
            done |= term | trunc
            if bool(done.all()):
                break
        env.errors()
        out = (total.cpu().tolist(), steps.cpu().tolist())
        if record:
            out = out + (torch.stack(acts).cpu(),)
        return out
    finally:
        env.close()


@torch.no_grad()
def evaluate_levels(ac, level_set, device="cuda", max_steps: int | None = None, chunk: int = 65536):
    """(rewards list[float], steps list[int]), entry l the deterministic episode from level l's start pose as
    evaluate_seeds reports it (the reward at the step the policy terminates, or 0.0 and max_steps when it does not
    within max_steps, default 4 * size^2): merlin.policy_field's predicted_episode on the set's maps.  Plain envs
    only: no stuck penalty, no exploration bonus."""
    from .policy_field import policy_field

    ls = level_set.to(device)
    ms = int(max_steps) if max_steps else 4 * ls.size * ls.size
    field = policy_field(ac, ls.walls.contiguous(), ls.goal.contiguous(), ls.size, chunk=chunk)
    reward, steps = field.predicted_episode(ls.agent.contiguous(), ms)
    return [float(r) for r in reward.cpu().tolist()], [int(s) for s in steps.cpu().tolist()]


@torch.no_grad()
def evaluate_zero_shot(ac, seeds, difficulty="mediumhard", size: int = 16, device="cuda",
                       max_steps: int | None = None, gamma: float = 0.995, lam: float = 0.95, **env_flags):
    """(rewards list[float], steps list[int], losses list[float]), one deterministic episode per
    seed, all at once (see the module docstring).  `difficulty`: one name, or one name per seed."""
    from . import _native as nat

    seeds = [int(s) for s in seeds]
    n = len(seeds)
    env = MerlinVecEnv(n, difficulty=_per_seed(difficulty, n), size=size, device=device, max_steps=max_steps, seeds=seeds,
                       **env_flags)
    try:
        obs = env.reset().clone()
        total = torch.zeros(n, dtype=torch.float64, device=env.device)
        steps = torch.zeros(n, dtype=torch.int64, device=env.device)
        done = torch.zeros(n, dtype=torch.bool, device=env.device)
        codes, acts, vals, rews = [], [], [], []
        for _ in range(env.max_steps):
            action, _, value = ac.act_codes(obs, deterministic=True)
            codes.append(obs.clone())
            acts.append(action)
            vals.append(value)
            obs, rew, term, trunc, info = env.step(action, autoreset=False)
            rews.append(rew.clone())
            live = ~done
            fin = live & (term | trunc)
            total = torch.where(fin, info["episode_return"], total)
            steps += live.long()
            done |= term | trunc
            if bool(done.all()):
                break
        env.errors()
    finally:
        env.close()
    T = len(acts)
    t_idx = torch.arange(T, device=steps.device).unsqueeze(1)
    valid = t_idx < steps.unsqueeze(0)  # [T, n]: the episode's own steps
    last = (t_idx == (steps - 1).unsqueeze(0)).float()  # done at the episode's last step: its bootstrap is masked
    V = torch.stack(vals).contiguous()
    adv, _ = nat.gae(torch.stack(rews).contiguous(), V, last.contiguous(), torch.zeros(n, device=V.device), gamma, lam)
    # per-episode normalisation (torch.std: unbiased), zeros for a one-step episode
    cnt = steps.clamp_min(1).to(torch.float32)
    a = torch.where(valid, adv, torch.zeros((), device=adv.device))
    mean = a.sum(0) / cnt
    var = torch.where(valid, (adv - mean) ** 2, torch.zeros((), device=adv.device)).sum(0) / (cnt - 1).clamp_min(1)
    adv_n = torch.where((steps > 1).unsqueeze(0), (adv - mean) / (var.sqrt() + 1e-8), torch.zeros((), device=adv.device))
    ret = V + adv_n
    # the episode's observations re-evaluated (policy.evaluate), every valid (t, env) at once
    sel = valid.reshape(-1)
    C = torch.stack(codes).reshape(T * n, -1)[sel]
    A = torch.stack(acts).reshape(-1)[sel]
    new_logp, _, new_v = ac.evaluate_codes(C, A)
    env_of = torch.arange(n, device=sel.device).repeat(T)[sel]
    lp_mean = torch.zeros(n, dtype=torch.float64, device=sel.device).index_add_(0, env_of, new_logp.double()) / cnt
    v_err = torch.zeros(n, dtype=torch.float64, device=sel.device).index_add_(
        0, env_of, ((new_v - ret.reshape(-1)[sel]) ** 2).double()) / cnt
    loss = (-lp_mean + 0.5 * v_err).float()
    return total.cpu().tolist(), steps.cpu().tolist(), loss.cpu().tolist()


def evaluate_few_shot(ac, seeds, adapt_steps: int, lr_inner: float = 0.01, k_support: int = 256,
                      difficulty="mediumhard", size: int = 16, device="cuda", max_steps: int | None = None,
                      task_batch: int = 32, **env_flags):
    """(rewards list[float], steps list[int], losses list[float]) of src/distribution_over_tasks.py:132-209 for
    many seeds: per seed, a copy of ``ac`` takes ``adapt_steps`` clipped SGD(lr_inner) steps, each on a fresh support
    rollout of ``k_support`` sampled steps of that seed's map, then plays one deterministic episode
    (merlin.few_shot.FewShotAdapter).  The seeds are processed ``task_batch`` at a time, the last chunk padded by
    repeating its last seed (its padded results dropped), so one rollout shape -- one HIP graph -- serves every chunk.
    adapt_steps = 0 scores ``ac`` itself, as evaluate_zero_shot does.  `difficulty`: one name, or one name per seed
    (the padding of the last chunk repeats the last seed's difficulty with it).

    The support rollouts' draws are keyed by a seed taken from torch's generator when this function starts, the
    rollout counter, the step and the task's position in its chunk: the same torch.manual_seed and the same calls
    give identical results, and moving a seed to another position (another task_batch) changes its draws."""
    from . import _native as nat
    from .few_shot import FewShotAdapter

    seeds = [int(s) for s in seeds]
    names = _per_seed(difficulty, len(seeds))
    rewards, steps, losses = [], [], []
    if not seeds:
        return rewards, steps, losses
    B = max(1, min(int(task_batch), len(seeds)))
    if isinstance(names, str):
        base, names = names, None
    else:  # the task envs are created on the lowest class listed; every chunk then sets its own classes
        for d in names:
            if d not in nat.DIFFICULTY_IDS:
                raise ValueError(f"Unknown difficulty: {d}")
        base = min(names, key=nat.DIFFICULTY_IDS.__getitem__)
    ad = FewShotAdapter(ac, lr_inner=lr_inner, difficulty=base, size=size, device=device, max_steps=max_steps,
                        **env_flags)
    try:
        for c0 in range(0, len(seeds), B):
            chunk = seeds[c0:c0 + B]
            m = len(chunk)
            chunk = chunk + [chunk[-1]] * (B - m)
            cls = None if names is None else names[c0:c0 + B] + [names[c0 + m - 1]] * (B - m)
            params = ad.adapt(chunk, int(adapt_steps), int(k_support), task_difficulties=cls)
            r, s, ls = ad.episode(params, chunk, task_difficulties=cls)
            rewards += r[:m]
            steps += s[:m]
            losses += ls[:m]
    finally:
        ad.close()
    return rewards, steps, losses


def evaluate_across_difficulties(ac, difficulties, num_tasks: int = 50, base_seed: int = 300000, adapt_steps: int = 0,
                                 **kw) -> dict:
    """{name: (rewards, steps, losses)} for each of `difficulties`, every one on the same seeds base_seed + i, i <
    num_tasks (the reference's cross-difficulty analyses: ppo/analyze_ppo_distribution.py collect_zero_shot_metrics,
    fomaml/analyze_fomaml_distribution.py collect_meta_metrics), in ONE batched pass over len(difficulties) *
    num_tasks envs of a mixed-task vector env instead of one pass per difficulty.  adapt_steps = 0: zero-shot
    (evaluate_zero_shot); > 0: after few-shot adaptation (evaluate_few_shot; lr_inner, k_support, task_batch in kw).
    The envs are laid out difficulty by difficulty, so num_tasks a multiple of 64 keeps every wave on one generator."""
    names = [str(d) for d in difficulties]
    if len(set(names)) != len(names):
        raise ValueError(f"a difficulty is listed twice: {names}")
    num_tasks = int(num_tasks)
    seeds = [int(base_seed) + i for i in range(num_tasks)] * len(names)
    per_seed = [d for d in names for _ in range(num_tasks)]
    if int(adapt_steps) > 0:
        res = evaluate_few_shot(ac, seeds, int(adapt_steps), difficulty=per_seed, **kw)
    else:
        for k in ("lr_inner", "k_support", "task_batch"):  # few-shot only
            kw.pop(k, None)
        res = evaluate_zero_shot(ac, seeds, difficulty=per_seed, **kw)
    return {d: tuple(x[j * num_tasks:(j + 1) * num_tasks] for x in res) for j, d in enumerate(names)}


def evaluate_policy(ac, difficulty: str = "mediumhard", episodes: int = 3, seed: int | None = None,
                    size: int = 16, device="cuda", max_steps: int | None = None, **env_flags):
    """Returns (rewards list[float], steps list[int]) like the reference's evaluate_policy."""
    base = 0 if seed is None else int(seed)
    return evaluate_seeds(ac, range(base, base + episodes), difficulty=difficulty, size=size, device=device,
                          max_steps=max_steps, **env_flags)


def sweep_checkpoints(model_dir: str, difficulty: str = "mediumhard", tasks: int = 50, size: int = 16,
                      device="cuda", **env_flags):
    """[(path, mean reward, mean steps)] of every *.pth in model_dir, best first
    (src/sweep_checkpoints.py:72-100)."""
    from .checkpoints import load_policy

    seeds = range(SWEEP_SEED_BASE, SWEEP_SEED_BASE + tasks)
    results = []
    for path in sorted(glob.glob(os.path.join(model_dir, "*.pth"))):
        policy = load_policy(path, device)
        rew, st = evaluate_seeds(policy, seeds, difficulty=difficulty, size=size, device=device, **env_flags)
        results.append((path, sum(rew) / len(rew), sum(st) / len(st)))
    results.sort(key=lambda r: r[1], reverse=True)
    return results
