"""Throughput of the full-grid render kernel (merlin_render_frames) against two yardsticks timed in the same process,
alternating call by call: (a) a plain torch fill of the same output tensor -- the write floor of this buffer on this
device -- and (b) the obvious torch formulation, atlas[tile_ids] gathered, permuted and made contiguous.

    python scripts/render_bench.py [--frames 256] [--size 16] [--tile_sizes 32,8] [--calls 30]

Prints one JSON line per tile size: the median milliseconds of each, frames/s and GB/s of the kernel, and its ratios.
The kernel must not be slower than (b) (exit status 1 if it is); the ratio to (a) is reported only.
DESIGN.md section 6c records the numbers.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ppo-2dgrid_amd"))

from merlin import MerlinVecEnv  # noqa: E402
from merlin import _native as nat  # noqa: E402


def tile_ids(walls, goal, agent, size, device):
    """int64[F, S, S] atlas indices WITHOUT the highlight (yardstick (b) is given the easier job: no view mask)."""
    F, S = agent.shape[0], size
    x = torch.arange(S, device=device)
    wall = ((walls[:, :, None] >> x[None, None, :]) & 1).long()  # [F, y, x]
    ids = wall.clone()
    f = torch.arange(F, device=device)
    gx, gy = goal[:, 0].long(), goal[:, 1].long()
    ids[f, gy, gx] = torch.where(wall[f, gy, gx] == 1, ids[f, gy, gx], torch.full_like(gx, 2))
    ax, ay, d = agent[:, 0].long(), agent[:, 1].long(), agent[:, 2].long()
    on_goal = ((ax == gx) & (ay == gy)).long()
    ids[f, ay, ax] = 6 + (on_goal * 4 + d) * 2
    return ids


def torch_render(atlas, ids, size, ts):
    F = ids.shape[0]
    return atlas[ids].permute(0, 1, 3, 2, 4, 5).contiguous().view(F, size * ts, size * ts, 3)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--size", type=int, default=16)
    p.add_argument("--tile_sizes", type=str, default="32,8")
    p.add_argument("--calls", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args(argv)
    dev = torch.device("cuda:0")
    F, S = args.frames, args.size
    env = MerlinVecEnv(F, difficulty="mediumhard", size=S, seed=1, device=dev)
    env.reset()
    walls, goal, agent = env.snapshot()
    env.close()
    ok = True
    for ts in [int(t) for t in args.tile_sizes.split(",")]:
        out = torch.empty((F, S * ts, S * ts, 3), dtype=torch.uint8, device=dev)
        atlas = torch.from_numpy(nat.frame_atlas(ts)).to(dev)
        ids = tile_ids(walls, goal, agent, S, dev)
        plain = nat.render_frames(walls, goal, agent, S, ts, False)
        assert torch.equal(torch_render(atlas, ids, S, ts), plain), "the torch formulation disagrees with the kernel"
        runs = {"kernel": lambda: nat.render_frames(walls, goal, agent, S, ts, True, out=out),
                "fill": lambda: out.fill_(7),
                "torch": lambda: torch_render(atlas, ids, S, ts)}
        events = {k: [] for k in runs}
        for it in range(args.warmup + args.calls):
            for k, fn in runs.items():  # alternating
                ev = timed(fn)
                if it >= args.warmup:
                    events[k].append(ev)
        torch.cuda.synchronize()
        ms = {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in events.items()}
        nbytes = out.numel()
        res = {"tile_size": ts, "frames": F, "size": S, "bytes": nbytes, "calls": args.calls,
               "kernel_ms": round(ms["kernel"], 4), "fill_ms": round(ms["fill"], 4), "torch_ms": round(ms["torch"], 4),
               "frames_per_s": round(F / ms["kernel"] * 1e3), "kernel_GBps": round(nbytes / ms["kernel"] / 1e6, 1),
               "fill_GBps": round(nbytes / ms["fill"] / 1e6, 1),
               "kernel_over_fill_bandwidth": round(ms["fill"] / ms["kernel"], 3),
               "torch_over_kernel_time": round(ms["torch"] / ms["kernel"], 2)}
        print(json.dumps(res), flush=True)
        ok = ok and ms["kernel"] <= ms["torch"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
