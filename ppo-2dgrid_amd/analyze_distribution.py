"""One policy scored across difficulties on the same seeds -- the reference's ppo/analyze_ppo_distribution.py
(zero-shot) and fomaml/analyze_fomaml_distribution.py (after few-shot adaptation) in one batched pass.

    python ppo-2dgrid_amd/analyze_distribution.py --model_path ppo.pth --difficulties easy medium hard
    python ppo-2dgrid_amd/analyze_distribution.py --model_path fomaml.pth --adapt_steps 3 --k_support 256

Every difficulty is played on the seeds base_seed .. base_seed + num_tasks - 1, all difficulties at once in one
mixed-task vector env (merlin.evaluation.evaluate_across_difficulties): zero-shot when --adapt_steps is 0, otherwise
after --adapt_steps clipped SGD(--lr_inner) steps per task on sampled support rollouts of --k_support steps.  Writes
one JSON file (--out): per difficulty the per-task rewards / steps / losses and their mean and std, and for every
pair of difficulties the distances of merlin.metrics.task_metrics between their (reward, steps) samples.  No plots.
--efficiency adds per difficulty an "efficiency" object: the path metrics of merlin.pathing (SPL, success rate, reward
against the optimum) and each task's shortest path length.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from merlin.checkpoints import load_policy  # noqa: E402
from merlin.evaluation import evaluate_across_difficulties  # noqa: E402
from merlin.metrics.task_metrics import compare_task_feature_dict  # noqa: E402
from merlin.scenario_creator import DEFAULT_CONFIG, ScenarioCreator  # noqa: E402
from merlin.utils.utils import get_device  # noqa: E402

ALL = ["easy", "medium", "mediumhard", "hard", "hardest"]


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--difficulties", type=str, nargs="+", default=ALL)
    p.add_argument("--num_tasks", type=int, default=50)
    p.add_argument("--base_seed", type=int, default=300000)
    p.add_argument("--config", type=str, default=DEFAULT_CONFIG)
    p.add_argument("--adapt_steps", type=int, default=0)
    p.add_argument("--k_support", type=int, default=256)
    p.add_argument("--lr_inner", type=float, default=0.01)
    p.add_argument("--task_batch", type=int, default=32, help="tasks adapted and scored at once (few-shot)")
    p.add_argument("--out", type=str, default="distribution_analysis.json")
    p.add_argument("--efficiency", action="store_true",
                   help="add SPL, success rate and reward ratio against each task's shortest path")
    return p.parse_args(argv)


def env_kwargs_of(sc: ScenarioCreator, difficulties):
    """({config name: generator}, the env kwargs the difficulties share); they may differ in the generator only."""
    gens, common = {}, None
    for d in difficulties:
        kw = sc._env_kwargs(d)
        gens[d] = kw.pop("difficulty")
        if common is None:
            common = kw
        elif kw != common:
            raise ValueError(f"difficulties {difficulties[0]} and {d} differ in size or params: one vector env "
                             "holds one grid size")
    if len(set(gens.values())) != len(gens):
        raise ValueError(f"two of {list(gens)} name the same generator")
    return gens, common


def add_efficiency(args, gens, env_kwargs, device, per):
    """per[d]["efficiency"]: path_metrics of d's episodes against the shortest paths of the same seeds (one kernel for
    all difficulties), and one printed line per difficulty."""
    from merlin.pathing import optimal_paths, path_metrics

    for flag in ("stuck_penalty", "exploration_bonus"):
        if env_kwargs.get(flag):
            raise ValueError(f"--efficiency: {flag} shapes the reward, and success is defined as reward > 0")
    kw = {k: env_kwargs[k] for k in ("size", "max_steps") if k in env_kwargs}
    nt = args.num_tasks
    seeds = [args.base_seed + i for i in range(nt)] * len(args.difficulties)
    opt, _ = optimal_paths(seeds, difficulty=[gens[d] for d in args.difficulties for _ in range(nt)], device=device,
                           **kw)
    size = int(kw.get("size", 16))
    max_steps = int(kw["max_steps"]) if kw.get("max_steps") else 4 * size * size
    for j, d in enumerate(args.difficulties):
        o = opt[j * nt:(j + 1) * nt]
        m = path_metrics(per[d]["rewards"], per[d]["steps"], o, max_steps)
        m.pop("per_task")
        m["opt_steps"] = o
        per[d]["efficiency"] = m
        print(f"    {d:<11} spl {m['spl']:.3f} | success {m['success_rate']:.3f} | reward ratio "
              f"{m['reward_ratio']:.3f} | {m['n_solvable']}/{m['n_tasks']} solvable")


def main(argv=None):
    args = parse_args(argv)
    device = get_device("auto")
    gens, env_kwargs = env_kwargs_of(ScenarioCreator(args.config), args.difficulties)
    policy = load_policy(args.model_path, device)
    shot = "zero-shot" if args.adapt_steps == 0 else f"{args.adapt_steps}-shot"
    print(f"[*] {os.path.basename(args.model_path)} | {shot} | {', '.join(args.difficulties)} | "
          f"{args.num_tasks} tasks from seed {args.base_seed}")
    t0 = time.time()
    few = dict(lr_inner=args.lr_inner, k_support=args.k_support, task_batch=args.task_batch)
    res = evaluate_across_difficulties(policy, [gens[d] for d in args.difficulties], num_tasks=args.num_tasks,
                                       base_seed=args.base_seed, adapt_steps=args.adapt_steps, device=device,
                                       **few, **env_kwargs)
    per, feats = {}, {}
    for d in args.difficulties:
        rew, steps, losses = res[gens[d]]
        per[d] = {"rewards": rew, "steps": steps, "losses": losses,
                  "reward_mean": float(np.mean(rew)), "reward_std": float(np.std(rew)),
                  "steps_mean": float(np.mean(steps)), "steps_std": float(np.std(steps))}
        feats[d] = np.stack([np.asarray(rew, dtype=np.float64), np.asarray(steps, dtype=np.float64)], axis=1)
        print(f"    {d:<11} reward {per[d]['reward_mean']:.3f} +- {per[d]['reward_std']:.3f} | "
              f"steps {per[d]['steps_mean']:.1f} +- {per[d]['steps_std']:.1f}")
    if args.efficiency:
        add_efficiency(args, gens, env_kwargs, device, per)
    pairs = {f"{a}|{b}": m for (a, b), m in compare_task_feature_dict(feats).items()}
    out = {"model_path": args.model_path, "difficulties": args.difficulties, "num_tasks": args.num_tasks,
           "base_seed": args.base_seed, "adapt_steps": args.adapt_steps, "lr_inner": args.lr_inner,
           "k_support": args.k_support, "per_difficulty": per, "pairwise": pairs}
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"[*] Complete in {time.time() - t0:.2f}s -> {args.out}")
    return out


if __name__ == "__main__":
    main()
