"""Where on a map a policy reaches the goal, and where it circles for ever -- the policy field (merlin/policy_field.py,
DESIGN.md 6e) of one checkpoint on the tasks the other analyses play.

    python ppo-2dgrid_amd/analyze_policy_field.py --model_path ppo.pth --difficulties easy medium hard --num_tasks 50

Every difficulty is taken on the seeds base_seed .. base_seed + num_tasks - 1 (analyze_distribution.py's tasks).  For
every free pose of every map -- not just the start pose -- the policy's argmax action is computed in one batched
forward, and one kernel follows those actions to the goal or into a cycle.  No episode is played.  Writes
<out_dir>/policy_field.json: per difficulty, under "field" the metrics over all solvable poses pooled (solved /
trapped / timeout rates, SPL, excess steps, the share of poses whose action is an optimal one, the critic's error) and
map by map, and under "start" the start-pose view of the same tasks: the reward and steps evaluate_seeds reports for
each seed, predicted from the field, and the shortest path's length.  Unless --no_plots, the first --maps_to_draw maps
of each difficulty are drawn to <out_dir>/<difficulty>_map<k>.png: the full-grid frame beside per-cell heatmaps of the
least steps over the four directions, the number of trapped directions and the greatest value.

    python ppo-2dgrid_amd/analyze_policy_field.py --model_path ppo.pth --difficulties medium --num_tasks 50 --sampled

--sampled adds what the policy does when it SAMPLES its actions, as training does (merlin/sampled_field.py, DESIGN.md
6f): per difficulty a "sampled" block with the metrics over all solvable poses (success rate, expected return and
steps, the regret against the shortest path, the critic's error against the sampled discounted return), under "start"
the probability of success and the expected reward and length of each seed's episode, and under
"length_distribution" the episode-length distribution pooled over the seeds -- all exact, from two dynamic programmes
over the policy's Markov chain, with no episode played.  Each drawn map then gains two heatmaps: the success
probability (greatest over directions) and the expected visits per cell (summed over directions).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from merlin.checkpoints import load_policy  # noqa: E402
from merlin.policy_field import policy_field_for_seeds  # noqa: E402
from merlin.sampled_field import sampled_field  # noqa: E402
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
    p.add_argument("--size", type=int, default=None, help="grid size (default: the config's)")
    p.add_argument("--gamma", type=float, default=0.99, help="discount of the return the critic is held against")
    p.add_argument("--out_dir", type=str, default="policy_field")
    p.add_argument("--no_plots", action="store_true")
    p.add_argument("--maps_to_draw", type=int, default=4, help="maps drawn per difficulty")
    p.add_argument("--sampled", action="store_true",
                   help="add the sampled policy's exact success / return / visits (merlin/sampled_field.py)")
    return p.parse_args(argv)


def sampled_block(sfield, agent, seeds):
    """(the "sampled" block of one difficulty, visits float64[M, 4, S, S]) of a SampledField and the start poses."""
    success, ret, steps = sfield.at(agent)
    visits, hit = sfield.occupancy(agent)
    pooled = hit.mean(dim=0)
    block = {"field": sfield.metrics(),
             "start": {"seeds": seeds, "success": success.cpu().tolist(), "ret": ret.cpu().tolist(),
                       "steps": steps.cpu().tolist()},
             # P(the episode of a seed drawn uniformly terminates at action t), t = 1..max_steps, and P(it is truncated)
             "length_distribution": {"terminated_at": pooled.cpu().tolist(), "truncated": float(1.0 - pooled.sum())}}
    return block, visits


def draw_maps(field, agent, name: str, k: int, out_dir: str, sampled=None) -> int:
    """<out_dir>/<name>_map<i>.png for the first k maps; 0 when matplotlib is missing.  sampled = (SampledField,
    visits): two more panels."""
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return 0
    from merlin import _native as nat

    k = min(int(k), field.n_maps)
    if k <= 0:
        return 0
    frames = nat.render_frames(field.walls[:k], field.goal[:k], agent[:k].contiguous(), field.size, tile_size=16).cpu()
    steps, free = field.steps[:k].float(), field.free[:k]
    nan = torch.full_like(steps, float("nan"))
    least = torch.where(steps >= 1, steps, torch.full_like(steps, float("inf"))).amin(dim=1)
    least = torch.where(torch.isinf(least), nan[:, 0], least).cpu()       # no direction arrives: blank
    trapped = torch.where(free[:, 0], ((steps == -1) & free).sum(dim=1).float(), nan[:, 0]).cpu()
    value = torch.where(free, field.value[:k], torch.full_like(steps, float("-inf"))).amax(dim=1)
    value = torch.where(torch.isinf(value), nan[:, 0], value).cpu()
    extra = []
    if sampled is not None:
        sfield, visits = sampled
        best = torch.nan_to_num(sfield.success[:k], nan=float("-inf")).amax(dim=1)
        best = torch.where(torch.isinf(best), nan[:, 0].to(best.dtype), best).cpu()
        seen = torch.where(free[:, 0], visits[:k].sum(dim=1), nan[:, 0].to(visits.dtype)).cpu()
        extra = [(best, "sampled: P(success) (greatest over directions)", "viridis"),
                 (seen, "sampled: expected visits (summed over directions)", "cividis")]
    for i in range(k):
        fig, ax = plt.subplots(1, 4 + len(extra), figsize=(18 + 4.5 * len(extra), 4.8))
        ax[0].imshow(frames[i].numpy())
        ax[0].set_title(f"{name} map {i}")
        panels = [(ax[1], least[i], "steps to the goal (least over directions)", "viridis_r"),
                  (ax[2], trapped[i], "trapped directions", "Reds"),
                  (ax[3], value[i], "value (greatest over directions)", "magma")]
        panels += [(ax[4 + j], img[i], title, cmap) for j, (img, title, cmap) in enumerate(extra)]
        for a, img, title, cmap in panels:
            im = a.imshow(img.numpy(), cmap=cmap, vmin=0 if a is ax[2] else None, vmax=4 if a is ax[2] else None)
            a.set_title(title)
            fig.colorbar(im, ax=a, fraction=0.046)
        for a in ax:
            a.set_xticks([])
            a.set_yticks([])
        fig.tight_layout()
        fig.savefig(os.path.join(out_dir, f"{name}_map{i}.png"), dpi=100)
        plt.close(fig)
    return k


def main(argv=None):
    args = parse_args(argv)
    device = get_device("auto")
    sc = ScenarioCreator(args.config)
    policy = load_policy(args.model_path, device)
    os.makedirs(args.out_dir, exist_ok=True)
    seeds = [args.base_seed + i for i in range(args.num_tasks)]
    print(f"[*] {os.path.basename(args.model_path)} | policy field | {', '.join(args.difficulties)} | "
          f"{args.num_tasks} tasks from seed {args.base_seed}")
    t0 = time.time()
    per, sizes, horizons = {}, set(), set()
    for d in args.difficulties:
        kw = sc._env_kwargs(d)
        for flag in ("stuck_penalty", "exploration_bonus"):
            if kw.get(flag):
                raise ValueError(f"{flag} shapes the reward: the field predicts unshaped episodes")
        size = int(args.size) if args.size else int(kw["size"])
        field, agent, ms = policy_field_for_seeds(policy, seeds, difficulty=kw["difficulty"], size=size, device=device,
                                                  max_steps=kw.get("max_steps"))
        sizes.add(size)
        horizons.add(ms)
        m = field.metrics(ms, gamma=args.gamma)
        rew, steps = field.predicted_episode(agent, ms)
        _, dist = field.at(agent)
        per[d] = {"field": m, "start": {"seeds": seeds, "rewards": rew.double().cpu().tolist(),
                                        "steps": steps.cpu().tolist(), "opt_steps": dist.cpu().tolist()}}
        print(f"    {d:<11} solved {m['solved_rate']:.3f} | trapped {m['trapped_rate']:.3f} | timeout "
              f"{m['timeout_rate']:.3f} | spl {m['spl']:.3f} | optimal actions {m['optimal_action_rate']:.3f} | "
              f"value rmse {m['value_rmse']:.3f} | {m['n_solvable']}/{m['n_free']} poses solvable")
        drawn = None
        if args.sampled:
            sfield = sampled_field(policy, field.walls, field.goal, size, ms, gamma=args.gamma)
            per[d]["sampled"], visits = sampled_block(sfield, agent, seeds)
            sm = per[d]["sampled"]["field"]
            print(f"    {'':<11} sampled: success {sm['success_rate']:.3f} | return {sm['expected_return']:.3f} | steps "
                  f"{sm['expected_steps']:.1f} | regret {sm['return_regret']:.3f} | value rmse "
                  f"{sm['value_rmse_sampled']:.3f}")
            drawn = (sfield, visits)
        if not args.no_plots:
            n = draw_maps(field, agent, d, args.maps_to_draw, args.out_dir, sampled=drawn)
            if n == 0 and args.maps_to_draw > 0:
                print("[*] matplotlib is not installed: maps not drawn")
    out = {"model_path": args.model_path, "difficulties": args.difficulties, "num_tasks": args.num_tasks,
           "base_seed": args.base_seed, "size": sizes.pop() if len(sizes) == 1 else sorted(sizes),
           "max_steps": horizons.pop() if len(horizons) == 1 else sorted(horizons), "gamma": args.gamma,
           "per_difficulty": per}
    path = os.path.join(args.out_dir, "policy_field.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(f"[*] Complete in {time.time() - t0:.2f}s -> {path}")
    return out


if __name__ == "__main__":
    main()
