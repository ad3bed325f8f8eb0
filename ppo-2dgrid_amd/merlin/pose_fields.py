"""What merlin/pathing.py, merlin/policy_field.py and merlin/sampled_field.py share: the free poses of
M maps in (map, dir, y, x) order, the lookup of one pose per map in an [M, 4, S, S] field, the maps of a list of seeds,
the distance field, the forward of a policy over every free pose, and the ratio reductions of the two ``metrics``."""
from __future__ import annotations

import contextlib

import torch

from . import _native as nat

VEC = ((1, 0), (0, 1), (-1, 0), (0, -1))  # DIR_TO_VEC: 0 = +x, 1 = +y, 2 = -x, 3 = -y


def free_cells(walls: torch.Tensor, size: int) -> torch.Tensor:
    """bool[M, S, S], indexed [y][x]: the cells of walls int32[M, S] (bit x of row y = wall) that are no wall."""
    x = torch.arange(int(size), device=walls.device, dtype=torch.int64)
    return ((walls.long().unsqueeze(-1) >> x) & 1) == 0


def free_poses(walls: torch.Tensor, size: int):
    """(agent int32[n, 4] = x, y, dir, 0, map_index int32[n]) on the walls' device: every free pose of every map, in
    (map, dir, y, x) order -- the row-major order of the [M, 4, S, S] fields."""
    S = int(size)
    free = free_cells(walls, S).unsqueeze(1).expand(-1, 4, -1, -1)
    m, d, y, x = free.nonzero(as_tuple=True)
    agent = torch.stack([x, y, d, torch.zeros_like(x)], dim=1).to(torch.int32).contiguous()
    return agent, m.to(torch.int32).contiguous()


class PoseField:
    """Base of the field dataclasses: they hold `size` and `walls` int32[M, S], all tensors on one device."""

    @property
    def n_maps(self) -> int:
        return int(self.walls.shape[0])

    def _lookup(self, agent: torch.Tensor):
        """(ok bool[M], index into an [M, 4, S, S] field) of pose agent[m] on map m; clamped where outside (ok False)."""
        S = self.size
        agent = agent.to(self.walls.device)
        if agent.shape != (self.n_maps, 4):
            raise ValueError(f"one pose per map: expected {self.n_maps}x4, got {tuple(agent.shape)}")
        x, y, d = agent[:, 0].long(), agent[:, 1].long(), agent[:, 2].long()
        ok = (x >= 0) & (x < S) & (y >= 0) & (y < S) & (d >= 0) & (d < 4)
        m = torch.arange(self.n_maps, device=agent.device)
        return ok, (m, d.clamp(0, 3), y.clamp(0, S - 1), x.clamp(0, S - 1))


@contextlib.contextmanager
def seeded_env(seeds, difficulty="mediumhard", size: int = 16, device="cuda", max_steps: int | None = None):
    """One seeded vector env on the maps evaluate_seeds plays for `seeds` (`difficulty`: one name, or one per seed),
    reset once; on leaving, its error flags are checked and it is closed."""
    from .envs import MerlinVecEnv
    from .evaluation import _per_seed

    seeds = [int(s) for s in seeds]
    n = len(seeds)
    env = MerlinVecEnv(n, difficulty=_per_seed(difficulty, n), size=size, device=device, max_steps=max_steps, seeds=seeds)
    try:
        env.reset()
        yield env
        env.errors()
    finally:
        env.close()


def maps_for_seeds(seeds, difficulty="mediumhard", size: int = 16, device="cuda", max_steps: int | None = None):
    """(walls int32[n, S], goal int32[n, 2], agent int32[n, 4], max_steps): the maps and start poses of `seeds` (one
    seeded_env, one snapshot) and the effective episode limit."""
    with seeded_env(seeds, difficulty, size, device, max_steps) as env:
        return (*env.snapshot(), int(env.max_steps))


def distance_field(walls: torch.Tensor, goal: torch.Tensor, size: int) -> torch.Tensor:
    """int16[M, 4, S, S]: the least number of actions any behaviour needs from every pose, -1: none
    (merlin_shortest_paths' field for device tensors, merlin_shortest_paths_host's for CPU tensors)."""
    zeros = torch.zeros((int(walls.shape[0]), 4), dtype=torch.int32, device=walls.device)
    if walls.is_cuda:
        return nat.shortest_paths(walls, goal, zeros, int(size), field=True)[1]
    return torch.from_numpy(nat.shortest_paths_host(walls.numpy(), goal.numpy(), zeros.numpy(), int(size), field=True)[1])


def over_free_poses(walls: torch.Tensor, goal: torch.Tensor, size: int, chunk: int, forward, outputs):
    """One view_codes launch over all free poses, `forward(codes[i:i + chunk])` -> one per-frame tensor per output, in
    chunks of `chunk` frames, and a scatter into [M, 4, S, S, ...] fields.  outputs: per field (dtype, the shape after
    [M, 4, S, S], the value where not free).  Returns (fields, codes int32[n, 8], agent int32[n, 4], map_index)."""
    S = int(size)
    M = int(walls.shape[0])
    agent, index = free_poses(walls, S)
    codes = nat.view_codes(walls, goal, agent, S, map_index=index)
    fields = [torch.full((M, 4, S, S, *shape), fill, dtype=dtype, device=walls.device) for dtype, shape, fill in outputs]
    where = (index.long(), agent[:, 2].long(), agent[:, 1].long(), agent[:, 0].long())
    step = max(int(chunk), 1)
    for i in range(0, int(agent.shape[0]), step):
        here = tuple(w[i:i + step] for w in where)
        for f, res in zip(fields, forward(codes[i:i + step])):
            f[here] = res.to(f.dtype)
    return fields, codes, agent, index


def ratio(v, den, per_map: bool = False) -> torch.Tensor:
    """sum(v) / sum(den) in float64 over the [M, 4, S, S] fields v and den: pooled over all maps (a scalar) or map by
    map (float64[M]); NaN where sum(den) is 0."""
    dims = (1, 2, 3) if per_map else None
    num, den = v.to(torch.float64).sum(dim=dims), den.sum(dim=dims).to(torch.float64)
    return torch.where(den > 0, num / den.clamp(min=1), torch.full_like(num, float("nan")))
