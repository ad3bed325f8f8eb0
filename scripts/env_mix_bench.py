"""Env-only steps/s of a mixed-task vector env against a uniform one ("Per-env difficulties").

    python scripts/env_mix_bench.py [--num-envs 4096] [--size 16] [--steps 512] [--repeats 5]

Random actions with auto-reset, single-step launches with the library's own look-ahead refills, for three
assignments of the same envs: uniform mediumhard; merlin.task_mix.assign(n, five equal weights), i.e. contiguous
runs on 64-env boundaries; the interleaved i % 5 assignment, where every wave holds all five generators.  Each
configuration is warmed up, then timed `repeats` times (device synchronise around `steps` step launches); the
configurations alternate inside every repeat.  The single-step loop is what a rollout issues, but its ~10-us kernels
leave the host's launch rate in the figure; the same steps as multi-step launches of `steps` steps each (the generator inside the step
kernel, no refill pass) are timed too, where only the device's time counts.  Prints one JSON line: per configuration
and launch form the median and all values.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppo-2dgrid_amd"))

import torch  # noqa: E402

from merlin import MerlinVecEnv  # noqa: E402
from merlin.task_mix import DIFFICULTIES, assign  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=64, help="episode cap: a reset every <= 64 steps per env")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("env_mix_bench measures on a GPU (HIP) device; none is visible")
    dev = torch.device("cuda", 0)
    n = args.num_envs
    configs = {
        "uniform_mediumhard": "mediumhard",
        "aligned_runs": assign(n, {d: 1 for d in DIFFICULTIES}),
        "interleaved": [DIFFICULTIES[i % 5] for i in range(n)],
    }
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = torch.randint(0, 3, (args.steps, n), generator=g, dtype=torch.int64).to(dev)
    obs = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    rew = torch.zeros(n, dtype=torch.float32, device=dev)
    done = torch.zeros(n, dtype=torch.float32, device=dev)
    envs = {}
    for name, diff in configs.items():
        env = MerlinVecEnv(n, difficulty=diff, size=args.size, seed=777, device=dev, max_steps=args.max_steps)
        env.reset()
        envs[name] = env

    def single(env):
        for t in range(args.steps):
            env.step_into(acts[t], obs, rew, None, None, done)

    MULTI = 16  # multi-step launches per timed window (one is only a few milliseconds)

    def multi(env):
        for _ in range(MULTI):
            env.step_into(acts, None, None, None, None, None, n_steps=args.steps, action_stride=n)

    forms = {"single_step_launches": single, "multi_step_launches": multi}
    work = {"single_step_launches": args.steps * n, "multi_step_launches": MULTI * args.steps * n}
    for env in envs.values():  # warm-up: code objects, every path a reset can take
        for run in forms.values():
            run(env)
    torch.cuda.synchronize(dev)
    rates = {f"{name}/{form}": [] for name in envs for form in forms}
    for _ in range(args.repeats):
        for form, run in forms.items():
            for name, env in envs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run(env)
                torch.cuda.synchronize(dev)
                rates[f"{name}/{form}"].append(work[form] / (time.perf_counter() - t0))
    for env in envs.values():
        env.errors()
    out = {"metric": "env-only steps/s, random actions, auto-reset", "num_envs": n, "size": args.size,
           "steps": args.steps, "max_steps": args.max_steps,
           "results": {k: {"median": round(statistics.median(v), 1), "all": [round(x, 1) for x in v]}
                       for k, v in rates.items()}}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
