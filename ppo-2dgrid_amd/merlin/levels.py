"""Finite level sets and level replay.

``LevelSet``      a bank of L maps with their start poses, in MerlinVecEnv.snapshot()'s layouts: built from seeds with
                  the env's own generators (level l is exactly the map of reset(seed=seeds[l])), or from hand-made
                  arrays, validated on the host; saved and loaded as .npz.
``LevelSampler``  the sampling weights over a bound set: uniform, or prioritized level replay (Jiang et al. 2021) --
                  rank-based score priority mixed with staleness, unseen levels sampled in proportion to their share.

MerlinVecEnv.set_levels binds a set to an env (every reset then takes a level of it), merlin.PPO(level_set=...,
level_sampler=...) trains on it, merlin.evaluation.evaluate_levels scores a policy on every level.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as nat


class LevelSet:
    """walls int32[L, size] bit rows (bit x of row y = wall at (x, y)), goal int32[L, 2], agent int32[L, 4] = (x, y,
    dir, 0): torch tensors on one device.  ``seeds`` / ``difficulties``: what the levels were built from, or None.
    Lineage (level editing, merlin/level_edit.py): ``generation`` int32[L], 0 for a seed-built, hand-made or loaded level,
    else the editing round that made it; ``parent`` int32[L], the slot its parent held in that round, -1 for none."""

    def __init__(self, walls: torch.Tensor, goal: torch.Tensor, agent: torch.Tensor, size: int, seeds=None,
                 difficulties=None, generation=None, parent=None):
        self.walls, self.goal, self.agent = walls, goal, agent
        n = int(walls.shape[0])
        self.generation = (torch.zeros(n, dtype=torch.int32, device=walls.device) if generation is None
                           else generation.to(device=walls.device, dtype=torch.int32))
        self.parent = (torch.full((n,), -1, dtype=torch.int32, device=walls.device) if parent is None
                       else parent.to(device=walls.device, dtype=torch.int32))
        self.size = int(size)
        self.seeds = None if seeds is None else [int(s) for s in seeds]
        self.difficulties = None if difficulties is None else [str(d) for d in difficulties]
        L = int(walls.shape[0])
        if not 1 <= L <= nat.MAX_LEVELS:
            raise ValueError(f"a level set holds 1..{nat.MAX_LEVELS} levels, got {L}")
        if tuple(walls.shape) != (L, self.size) or tuple(goal.shape) != (L, 2) or tuple(agent.shape) != (L, 4):
            raise ValueError("LevelSet: walls [L, size], goal [L, 2], agent [L, 4]")
        if tuple(self.generation.shape) != (L,) or tuple(self.parent.shape) != (L,):
            raise ValueError("LevelSet: generation [L], parent [L]")

    def __len__(self) -> int:
        return int(self.walls.shape[0])

    @property
    def device(self):
        return self.walls.device

    def to(self, device) -> "LevelSet":
        dev = torch.device(device)
        if dev == self.device:
            return self
        return LevelSet(self.walls.to(dev), self.goal.to(dev), self.agent.to(dev), self.size, self.seeds,
                        self.difficulties, self.generation.to(dev), self.parent.to(dev))

    def replace_(self, slots: torch.Tensor, children: "LevelSet", generation, parent: torch.Tensor) -> None:
        """Child j of `children` takes slot slots[j] in place, with lineage (generation: one int or int32[C]; parent
        int32[C]); a slot < 0 drops its child.  A masked scatter into the existing tensors, no host sync: every holder of
        this set (the trainer, the env's mirror, an evaluation) sees the new levels.  Distinct slots >= 0 are the
        caller's to guarantee."""
        L = len(self)
        slots = slots.to(torch.int64)
        idx = torch.where(slots >= 0, slots, torch.full_like(slots, L))  # a dropped child lands in a spare row
        gen = torch.as_tensor(generation, dtype=torch.int32, device=slots.device).expand(slots.shape)
        for dst, src in ((self.walls, children.walls), (self.goal, children.goal), (self.agent, children.agent),
                         (self.generation, gen), (self.parent, parent)):
            tmp = torch.cat([dst, dst[:1]])
            tmp[idx] = src.to(dst.dtype)
            dst.copy_(tmp[:L])

    @classmethod
    def from_seeds(cls, seeds, difficulty="mediumhard", difficulties=None, size: int = 16, device="cuda") -> "LevelSet":
        """Level l = the map and start pose of reset(seed=seeds[l]) under `difficulty` (one name) or
        `difficulties` (one name per seed): a temporary vector env of L envs, seeded, reset and snapshotted -- the
        existing generators, nothing restated."""
        from .envs import MerlinVecEnv

        seeds = [int(s) for s in seeds]
        names = [str(difficulty)] * len(seeds) if difficulties is None else [str(d) for d in difficulties]
        if len(names) != len(seeds):
            raise ValueError(f"difficulties: {len(names)} names for {len(seeds)} seeds")
        uniform = len(set(names)) == 1
        env = MerlinVecEnv(len(seeds), difficulty=names[0] if uniform else names, size=size, device=device, seeds=seeds)
        try:
            env.reset()
            walls, goal, agent = env.snapshot()
            env.errors()
        finally:
            env.close()
        return cls(walls, goal, agent, size, seeds=seeds, difficulties=names)

    @classmethod
    def from_arrays(cls, walls, goal, agent, device=None, solvable: bool = False) -> "LevelSet":
        """Hand-made maps: walls [L, size] bit rows, goal [L, 2], agent [L, 3 or 4] = (x, y, dir[, 0]).  Checked on
        the host: size in 5..32, no bit beyond the grid, the border walled, agent and goal on distinct free cells,
        dir in 0..3; with `solvable` also that the goal can be reached (merlin_shortest_paths_host).  A ValueError
        names the first level that fails.  device None keeps the set on the CPU (.to(device) moves it)."""
        w = np.asarray(walls)
        g = np.asarray(goal)
        a = np.asarray(agent)
        if w.ndim != 2 or not 5 <= w.shape[1] <= 32:
            raise ValueError("from_arrays: walls is [L, size] with size in 5..32")
        L, S = int(w.shape[0]), int(w.shape[1])
        if L < 1:
            raise ValueError("from_arrays: no level")
        if g.shape != (L, 2) or a.ndim != 2 or a.shape[0] != L or a.shape[1] not in (3, 4):
            raise ValueError("from_arrays: goal is [L, 2], agent [L, 3] or [L, 4]")
        if not (np.issubdtype(w.dtype, np.integer) and np.issubdtype(g.dtype, np.integer)
                and np.issubdtype(a.dtype, np.integer)):
            raise ValueError("from_arrays: integer arrays")
        w = w.astype(np.int64) & 0xFFFFFFFF
        full = (1 << S) - 1
        edge = 1 | (1 << (S - 1))
        for l in range(L):
            if (w[l] & ~full).any():
                raise ValueError(f"level {l}: a wall bit beyond column {S - 1}")
            if w[l, 0] != full or w[l, S - 1] != full or ((w[l] & edge) != edge).any():
                raise ValueError(f"level {l}: the border is not walled")
            ax, ay, d = (int(v) for v in a[l, :3])
            gx, gy = (int(v) for v in g[l])
            if not (0 <= ax < S and 0 <= ay < S) or (w[l, ay] >> ax) & 1:
                raise ValueError(f"level {l}: the agent ({ax}, {ay}) is not on a free cell")
            if not (0 <= gx < S and 0 <= gy < S) or (w[l, gy] >> gx) & 1:
                raise ValueError(f"level {l}: the goal ({gx}, {gy}) is not on a free cell")
            if (ax, ay) == (gx, gy):
                raise ValueError(f"level {l}: the agent stands on the goal")
            if not 0 <= d <= 3:
                raise ValueError(f"level {l}: direction {d} outside 0..3")
        w32 = w.astype(np.uint32).view(np.int32).reshape(L, S)
        g32 = np.ascontiguousarray(g.astype(np.int32))
        a32 = np.zeros((L, 4), dtype=np.int32)
        a32[:, :3] = a[:, :3]
        if solvable:
            dist = nat.shortest_paths_host(np.ascontiguousarray(w32), g32, a32, S)
            bad = np.nonzero(dist < 0)[0]
            if bad.size:
                raise ValueError(f"level {int(bad[0])}: the goal cannot be reached")
        dev = torch.device("cpu" if device is None else device)
        return cls(torch.from_numpy(np.ascontiguousarray(w32)).to(dev), torch.from_numpy(g32).to(dev),
                   torch.from_numpy(a32).to(dev), S)

    def save(self, path: str) -> None:
        extra = {}
        if self.seeds is not None:
            extra["seeds"] = np.asarray(self.seeds, dtype=np.uint64)
        if self.difficulties is not None:
            extra["difficulties"] = np.asarray(self.difficulties)
        np.savez(path, walls=self.walls.cpu().numpy(), goal=self.goal.cpu().numpy(), agent=self.agent.cpu().numpy(),
                 size=np.int32(self.size), generation=self.generation.cpu().numpy(), parent=self.parent.cpu().numpy(),
                 **extra)

    @classmethod
    def load(cls, path: str, device=None) -> "LevelSet":
        """A saved set, validated again as from_arrays validates (a file is input like any other)."""
        with np.load(path, allow_pickle=False) as z:
            ls = cls.from_arrays(z["walls"], z["goal"], z["agent"], device=device)
            if int(z["size"]) != ls.size:
                raise ValueError(f"{path}: size {int(z['size'])} but rows of {ls.size}")
            if "seeds" in z.files:
                ls.seeds = [int(s) for s in z["seeds"]]
            if "difficulties" in z.files:
                ls.difficulties = [str(d) for d in z["difficulties"]]
            for name in ("generation", "parent"):  # lineage: files written before level editing have none
                if name in z.files:
                    v = np.asarray(z[name])
                    if v.shape != (len(ls),) or not np.issubdtype(v.dtype, np.integer):
                        raise ValueError(f"{path}: {name} is int[{len(ls)}]")
                    getattr(ls, name).copy_(torch.from_numpy(v.astype(np.int32)))
        return ls


class LevelSampler:
    """The sampling weights over L levels, every tensor of length L on `device`.

    update(sum, count, iteration)  the int64 vectors of merlin_level_scores: a level with count > 0 takes this
                                   rollout's step-weighted mean score, sum / count / 2^24 in float64, and last_seen =
                                   iteration.
    cdf()                          float64[L], non-decreasing, last entry exactly 1.0.  'uniform': (l + 1) / L.
                                   'plr': the seen levels ranked by score, descending, ties to the lower index; P_S ~
                                   rank^(-1/beta); P_C ~ iteration - last_seen (dropped where that sums to 0: every seen
                                   level was seen this iteration); P_seen = (1 - rho) P_S + rho P_C.  The seen levels
                                   share |seen| / L as P_seen, the unseen ones share the rest uniformly (1 / L each):
                                   the proportionate replay schedule.
    forget(slots)                  the slots >= 0 become unseen (score 0, last_seen 0): a level that was replaced.  An
                                   unseen level has weight 1 / L under the proportionate schedule.
    No host sync in any."""

    def __init__(self, L: int, strategy: str = "uniform", beta: float = 0.1, rho: float = 0.1,
                 score: str = "l1_value", device="cuda"):
        if strategy not in ("uniform", "plr"):
            raise ValueError(f"Unknown level replay strategy: {strategy}")
        if score not in nat.LEVEL_SCORE_KINDS:
            raise ValueError(f"Unknown level score: {score}")
        if not 1 <= int(L) <= nat.MAX_LEVELS:
            raise ValueError(f"1..{nat.MAX_LEVELS} levels, got {L}")
        if not beta > 0 or not 0.0 <= rho <= 1.0:
            raise ValueError("beta > 0 and rho in [0, 1]")
        self.L, self.strategy, self.beta, self.rho, self.score_kind = int(L), strategy, float(beta), float(rho), score
        dev = torch.device(device)
        self.score = torch.zeros(self.L, dtype=torch.float64, device=dev)
        self.last_seen = torch.zeros(self.L, dtype=torch.int64, device=dev)
        self.seen = torch.zeros(self.L, dtype=torch.bool, device=dev)
        self.iteration = 0

    def update(self, sum: torch.Tensor, count: torch.Tensor, iteration: int) -> None:
        now = count > 0
        mean = sum.double() / count.clamp_min(1).double() / nat.LEVEL_SCORE_SCALE
        self.score = torch.where(now, mean, self.score)
        self.last_seen = torch.where(now, torch.full_like(self.last_seen, int(iteration)), self.last_seen)
        self.seen = self.seen | now
        self.iteration = int(iteration)

    def forget(self, slots: torch.Tensor) -> None:
        slots = slots.to(torch.int64)
        hit = torch.zeros(self.L + 1, dtype=torch.bool, device=self.score.device)
        hit[torch.where(slots >= 0, slots, torch.full_like(slots, self.L))] = True  # -1 lands in the spare entry
        hit = hit[:self.L]
        self.score = torch.where(hit, torch.zeros_like(self.score), self.score)
        self.last_seen = torch.where(hit, torch.zeros_like(self.last_seen), self.last_seen)
        self.seen = self.seen & ~hit

    def weights(self) -> torch.Tensor:
        """float64[L]: the probability of each level (sums to 1 up to rounding)."""
        L = self.L
        dev = self.score.device
        if self.strategy == "uniform":
            return torch.full((L,), 1.0 / L, dtype=torch.float64, device=dev)
        seen = self.seen
        ns = seen.sum().double()
        # descending, stable: equal scores keep index order; the unseen levels sort behind every seen one
        key = torch.where(seen, self.score, torch.full_like(self.score, -float("inf")))
        order = torch.sort(key, descending=True, stable=True).indices
        rank = torch.empty(L, dtype=torch.float64, device=dev)
        rank[order] = torch.arange(1, L + 1, dtype=torch.float64, device=dev)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        w_s = torch.where(seen, rank.pow(-1.0 / self.beta), zero)
        p_s = w_s / w_s.sum().clamp_min(1e-300)
        w_c = torch.where(seen, (self.iteration - self.last_seen).double(), zero)
        tot_c = w_c.sum()
        p_seen = torch.where(tot_c > 0, (1.0 - self.rho) * p_s + self.rho * w_c / tot_c.clamp_min(1.0), p_s)
        return torch.where(seen, p_seen * (ns / L), torch.full_like(p_seen, 1.0 / L))

    def cdf(self) -> torch.Tensor:
        if self.strategy == "uniform":
            c = torch.arange(1, self.L + 1, dtype=torch.float64, device=self.score.device) / self.L
        else:
            # (a parallel scan may round neighbouring prefixes differently: keep the sequence monotone and <= 1)
            c = torch.cummax(torch.cumsum(self.weights(), 0).clamp_max(1.0), 0).values
        c[-1] = 1.0
        return c
