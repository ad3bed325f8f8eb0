"""Probe: what level editing costs.
1. merlin_levels_mutate at C = 64 and 512 (S = 16, E = 4, seed-built mediumhard parents) next to merlin_shortest_paths
   on the same children: the two run the same search, so that is the yardstick.  HIP events around `reps` launches.
2. One LevelEditor.evolve call end to end (selection, the kernel, the three in-place updates), host clock around the
   call with a device sync on both sides.
3. The benched rollout (4096 envs x 256 steps, the captured graph) on a bank of K levels under prioritized replay, with
   and without a replacement of C slots between rollouts, alternated in one process as scripts/probe_levels.py does.
    python scripts/probe_level_edit.py [K] [rollouts per block] [blocks]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-2dgrid_amd"))
import torch

from merlin import MerlinVecEnv
from merlin import _native as nat
from merlin.level_edit import LevelEditor, mutate_levels
from merlin.levels import LevelSampler, LevelSet
from merlin.ppo import PPO

N, T = 4096, 256


def per_call_us(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device("cuda", 0)
    ls = LevelSet.from_seeds(range(K), difficulty="mediumhard", size=16, device=dev)

    for Cn in (64, 512):
        pidx = (torch.arange(Cn, device=dev) % K).to(torch.int32)
        kids, dist, changed = mutate_levels(ls, pidx, 4, 777, 1)
        out = (kids.walls, kids.goal, kids.agent, dist, changed)
        for rep in (200, 200):
            m = per_call_us(lambda: nat.levels_mutate(ls.walls, ls.goal, ls.agent, pidx, 16, 4, 777, 1, out=out), rep)
            p = per_call_us(lambda: nat.shortest_paths(kids.walls, kids.goal, kids.agent, 16), rep)
            print(f"C = {Cn}: merlin_levels_mutate {m:.1f} us per call, merlin_shortest_paths on its children "
                  f"{p:.1f} us (changed {int(changed.sum())}, unsolvable {int((dist < 0).sum())})")

    env = MerlinVecEnv(N, difficulty="mediumhard", size=16, seed=777, device=dev)
    torch.manual_seed(777)
    Cn = max(1, K // 8)
    editor = LevelEditor(Cn, edits=4, seed=777)
    agent = PPO(env, lr=3e-4, gamma=0.99, lam=0.95, clip_eps=0.2, update_epochs=1, batch_size=N * T,
                minibatch_size=N * T // 8, vf_coef=0.5, ent_coef=0.05, device=dev, level_set=ls,
                level_sampler=LevelSampler(K, "plr", device=dev), level_seed=777)
    agent.update(agent.collect_rollouts())  # eager rollout + capture, an update: the scores are in
    assert agent._graph is not None
    sm = agent.level_sampler

    def rollouts(n, replace):
        times = []
        for _ in range(n):
            if replace:  # what an editing round does to the env, between two rollouts
                editor.evolve(agent.level_set, sm, agent.vec, 1)
                agent.vec.set_level_cdf(sm.cdf())
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            agent.collect_rollouts()
            torch.cuda.synchronize(dev)
            times.append((time.perf_counter() - t0) * 1e3)
        return times

    ev = []
    for _ in range(12):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        editor.evolve(agent.level_set, sm, agent.vec, 1)
        torch.cuda.synchronize(dev)
        ev.append((time.perf_counter() - t0) * 1e3)
        # score what is there again, so the next round has seen levels to choose from
        s, c = nat.level_scores(agent.buf.adv, agent.buf.levels, K, sm.score_kind)
        sm.update(s, c, sm.iteration + 1)
    ev = sorted(ev[2:])
    print(f"LevelEditor.evolve, L = {K}, C = {Cn}, E = 4: median {ev[len(ev) // 2]:.2f} ms, min {ev[0]:.2f}, max "
          f"{ev[-1]:.2f} (10 calls; accepted so far {int(editor.accepted.item())}, unsolvable "
          f"{int(editor.rejected_unsolvable.item())}, unchanged {int(editor.rejected_unchanged.item())})")

    rollouts(2, False)
    times = {False: [], True: []}
    for _ in range(blocks):
        for replace in (False, True):
            times[replace] += rollouts(per, replace)
            s, c = nat.level_scores(agent.buf.adv, agent.buf.levels, K, sm.score_kind)
            sm.update(s, c, sm.iteration + 1)
    for replace, t in times.items():
        t = sorted(t)
        name = "a replacement before each" if replace else "no replacement"
        print(f"rollout, levels K = {K} plr, {name}: median {t[len(t) // 2]:.2f} ms, min {t[0]:.2f}, max {t[-1]:.2f} "
              f"({len(t)} rollouts)")
    bank = agent.vec.level_bank()
    held = agent.level_set
    assert all((a == b).all() for a, b in zip(bank, (held.walls, held.goal, held.agent)))
    print(f"edited share of the bank {float((agent.level_set.generation > 0).double().mean()):.3f}, one graph: "
          f"{agent._graph is not None}")
    env.errors()


if __name__ == "__main__":
    main()
