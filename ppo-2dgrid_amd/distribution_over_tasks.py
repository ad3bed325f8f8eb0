"""PPO-vs-FOMAML evaluation over unseen tasks -- drop-in for the reference's src/distribution_over_tasks.py
(flags :24-36, plus --task_batch).

    python ppo-2dgrid_amd/distribution_over_tasks.py --ppo_model ppo.pth --fomaml_model fomaml.pth --adapt_steps 3

Tasks are the seeds base_seed .. base_seed + num_tasks - 1.  The PPO policy is scored zero-shot; the FOMAML policy
zero-shot when --adapt_steps is 0, otherwise after --adapt_steps clipped SGD steps per task on sampled support
rollouts (merlin.evaluation.evaluate_few_shot, --task_batch tasks at a time on the GPU envs).  Written to
<out_dir>/<ppo>_vs_<fomaml>/seed_<base>/<zero_shot | N_shot>/: results.json (per-task rewards, steps and losses of
both policies, the reward-distribution metrics of merlin.metrics.task_metrics, both mean rewards) and, when
matplotlib is installed, the reward / steps / loss histograms.
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
from merlin.evaluation import evaluate_few_shot, evaluate_zero_shot  # noqa: E402
from merlin.metrics.task_metrics import compare_two_feature_sets  # noqa: E402
from merlin.scenario_creator import DEFAULT_CONFIG, ScenarioCreator  # noqa: E402
from merlin.utils.utils import get_device  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--difficulty", type=str, default="mediumhard")
    p.add_argument("--num_tasks", type=int, default=500)
    p.add_argument("--ppo_model", type=str, required=True)
    p.add_argument("--fomaml_model", type=str, required=True)
    p.add_argument("--adapt_steps", type=int, default=0)
    p.add_argument("--lr_inner", type=float, default=0.01)
    p.add_argument("--k_support", type=int, default=256)
    p.add_argument("--config", type=str, default=DEFAULT_CONFIG)
    p.add_argument("--out_dir", type=str, default="eval_results")
    p.add_argument("--base_seed", type=int, default=100000)
    p.add_argument("--task_batch", type=int, default=32, help="tasks adapted and scored at once")
    return p.parse_args(argv)


def plot_histograms(ppo_data, fomaml_data, metric_name, out_path, total_tasks, title_suffix) -> bool:
    """Both policies' histogram of one per-task quantity on shared bins; False when matplotlib is missing."""
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    a = [x for x in ppo_data if np.isfinite(x)]
    b = [x for x in fomaml_data if np.isfinite(x)]
    if not a or not b:
        return True
    fig, ax = plt.subplots(figsize=(10, 6))
    bins = np.histogram_bin_edges(a + b, bins=50)
    ax.hist(a, bins=bins, alpha=0.5, label="BASE (PPO)")
    ax.hist(b, bins=bins, alpha=0.7, label="FOMAML")
    ax.set_xlabel(metric_name)
    ax.set_ylabel("Number of Tasks")
    ax.set_title(f"Distribution of {metric_name} ({title_suffix})")
    ax.set_ylim(0, total_tasks)
    ax.legend(loc="upper right")
    ax.grid(axis="y", alpha=0.4, linestyle="--")
    fig.tight_layout()
    fig.savefig(out_path, dpi=200, bbox_inches="tight")
    plt.close(fig)
    return True


def main(argv=None):
    args = parse_args(argv)
    device = get_device("auto")
    env_kwargs = ScenarioCreator(args.config)._env_kwargs(args.difficulty)
    ppo_name = os.path.splitext(os.path.basename(args.ppo_model))[0]
    fomaml_name = os.path.splitext(os.path.basename(args.fomaml_model))[0]
    shot = "zero_shot" if args.adapt_steps == 0 else f"{args.adapt_steps}_shot"
    out_dir = os.path.join(args.out_dir, f"{ppo_name}_vs_{fomaml_name}", f"seed_{args.base_seed}", shot)
    os.makedirs(out_dir, exist_ok=True)
    seeds = list(range(args.base_seed, args.base_seed + args.num_tasks))
    ppo_policy = load_policy(args.ppo_model, device)
    fomaml_policy = load_policy(args.fomaml_model, device)
    print(f"[*] Evaluation | {ppo_name} vs {fomaml_name} | {shot.replace('_', '-').upper()}")
    print(f"[*] Saving to: {out_dir}\n")
    t0 = time.time()
    ppo = evaluate_zero_shot(ppo_policy, seeds, device=device, **env_kwargs)
    if args.adapt_steps == 0:
        fom = evaluate_zero_shot(fomaml_policy, seeds, device=device, **env_kwargs)
    else:
        fom = evaluate_few_shot(fomaml_policy, seeds, args.adapt_steps, lr_inner=args.lr_inner,
                                k_support=args.k_support, device=device, task_batch=args.task_batch, **env_kwargs)
    metrics = compare_two_feature_sets(np.array(ppo[0]).reshape(-1, 1), np.array(fom[0]).reshape(-1, 1))
    title = "Zero-Shot" if args.adapt_steps == 0 else f"{args.adapt_steps}-Shot"
    print(f"--- Reward Distribution Shift ({title}) ---")
    for k, v in metrics.items():
        print(f"    {k:<20}: {v:.6f}")
    results = {
        "difficulty": args.difficulty, "base_seed": args.base_seed, "num_tasks": args.num_tasks,
        "adapt_steps": args.adapt_steps, "lr_inner": args.lr_inner, "k_support": args.k_support,
        "ppo_rewards": ppo[0], "ppo_steps": ppo[1], "ppo_losses": ppo[2],
        "fomaml_rewards": fom[0], "fomaml_steps": fom[1], "fomaml_losses": fom[2],
        "reward_metrics": metrics,
        "ppo_mean_reward": float(np.mean(ppo[0])), "fomaml_mean_reward": float(np.mean(fom[0])),
    }
    with open(os.path.join(out_dir, "results.json"), "w") as f:
        json.dump(results, f, indent=1)
    for i, (name, fname) in enumerate((("Reward", "reward_dist.png"), ("Steps to Goal", "steps_dist.png"),
                                       ("Validation Loss", "loss_dist.png"))):
        if not plot_histograms(ppo[i], fom[i], name, os.path.join(out_dir, fname), args.num_tasks, title):
            print("[*] matplotlib is not installed: histograms skipped")
            break
    print(f"\n[*] Complete in {time.time() - t0:.2f}s. PPO Avg Rew: {results['ppo_mean_reward']:.3f} | "
          f"FOMAML Avg Rew: {results['fomaml_mean_reward']:.3f}")
    return results


if __name__ == "__main__":
    main()
