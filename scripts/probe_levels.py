"""Probe: what level mode costs the rollout.  The benched rollout (4096 envs x 256 steps, mediumhard
16x16, the captured graph) on the default path -- endless generation on the map ring -- against the same rollout on a
bank of K levels under prioritized level replay, alternated in one process after one update each (so the replay
weights are prioritized, not uniform); and the scores kernel on the rollout's [256][4096] advantages.  A rollout's
time is a host clock around collect_rollouts() (which ends in host reads: episodes, error word), the kernel's is HIP
events around `reps` launches.
    python scripts/probe_levels.py [K] [rollouts per block] [blocks]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-2dgrid_amd"))
import torch

from merlin import MerlinVecEnv
from merlin import _native as nat
from merlin.levels import LevelSampler, LevelSet
from merlin.ppo import PPO

N, T = 4096, 256


def agent_of(dev, K):
    env = MerlinVecEnv(N, difficulty="mediumhard", size=16, seed=777, device=dev)
    torch.manual_seed(777)
    kw = {}
    if K:
        kw = dict(level_set=LevelSet.from_seeds(range(K), difficulty="mediumhard", size=16, device=dev),
                  level_sampler=LevelSampler(K, "plr", device=dev), level_seed=777)
    return PPO(env, lr=3e-4, gamma=0.99, lam=0.95, clip_eps=0.2, update_epochs=1, batch_size=N * T,
               minibatch_size=N * T // 8, vf_coef=0.5, ent_coef=0.05, device=dev, **kw)


def rollouts(agent, n, dev):
    times = []
    for _ in range(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        agent.collect_rollouts()
        torch.cuda.synchronize(dev)
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device("cuda", 0)
    agents = {"default": agent_of(dev, 0), f"levels K={K} plr": agent_of(dev, K)}
    for name, a in agents.items():  # eager rollout + capture, an update, two replays
        a.update(a.collect_rollouts())
        rollouts(a, 2, dev)
        assert a._graph is not None, name
    times = {name: [] for name in agents}
    for _ in range(blocks):
        for name, a in agents.items():
            times[name] += rollouts(a, per, dev)
    for name, t in times.items():
        t = sorted(t)
        print(f"rollout {name}: median {t[len(t) // 2]:.2f} ms, min {t[0]:.2f}, max {t[-1]:.2f} ({len(t)} rollouts)")
    lv = agents[f"levels K={K} plr"]
    sm = lv.level_sampler
    print(f"levels seen {int(sm.seen.sum())}/{K}, weights min {float(sm.weights().min()):.3e} max "
          f"{float(sm.weights().max()):.3e}, episodes in the last rollout {int((lv.buf.dones > 0).sum())}")
    adv, levels = lv.buf.adv, lv.buf.levels
    s = torch.empty(K, dtype=torch.int64, device=dev)
    c = torch.empty(K, dtype=torch.int64, device=dev)
    for reps in (50, 50):
        nat.level_scores(adv, levels, K, 0, sum=s, count=c)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            nat.level_scores(adv, levels, K, 0, sum=s, count=c)
        e1.record()
        torch.cuda.synchronize(dev)
        us = e0.elapsed_time(e1) / reps * 1e3
        print(f"merlin_level_scores [256][4096], L = {K} (zero + reduce, 2 launches): {us:.1f} us per call, "
              f"{N * T * 8 / us / 1e3:.0f} GB/s of adv + levels read")
    assert int(c.sum()) == N * T


if __name__ == "__main__":
    main()
