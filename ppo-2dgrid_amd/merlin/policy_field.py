"""The policy field: a deterministic policy's fate from every pose of a map.

Every ``evaluate_*`` function looks at a policy through one start pose per seed.  Two facts make the whole map
available at the price of one forward: the policy is a function of the 7x7 view codes only and ``evaluate_seeds`` acts
with the argmax, and the view is a function of (map, pose) only -- the step count is not observed.  So a policy turns
a map into a functional graph over its 4 S^2 poses, and the number of actions after which an episode started in a pose
terminates is one backward search over that graph; no rollout is played.

``free_poses``             every free pose of every map, in (map, dir, y, x) order.
``policy_field``           codes of all free poses (merlin._native.view_codes) -> the policy's argmax and value
                           (``ac.act_codes``, the call evaluate_seeds makes) -> steps (merlin._native.policy_paths) and
                           the shortest-path field dist beside it (merlin._native.shortest_paths).
``policy_field_for_seeds`` the same on the maps evaluate_seeds plays for a list of seeds, with their start poses.
``PolicyField``            ``at`` (lookup), ``predicted_episode`` (what evaluate_seeds will report from a pose) and
                           ``metrics`` (solved / trapped / timeout rates, SPL, excess steps, the share of optimal
                           actions and the critic's error over the solvable poses).

steps: -1 = the episode never terminates (a cycle, a forward move into a wall, or a pose leading to one); no horizon
is applied, callers compare with max_steps.  Only the three native entries are kernels; the rest is torch.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _native as nat
from .pathing import optimal_reward
from .pose_fields import (PoseField, distance_field, free_cells, free_poses, maps_for_seeds,  # noqa: F401
                          over_free_poses, ratio)


def _front(t: torch.Tensor, fill):
    """t[M, 4, S, S] read at each pose's front cell (same direction), `fill` where that is off the grid."""
    out = torch.full_like(t, fill)
    out[:, 0, :, :-1] = t[:, 0, :, 1:]
    out[:, 1, :-1, :] = t[:, 1, 1:, :]
    out[:, 2, :, 1:] = t[:, 2, :, :-1]
    out[:, 3, 1:, :] = t[:, 3, :-1, :]
    return out


@dataclass
class PolicyField(PoseField):
    """All tensors on one device; the [M, 4, S, S] fields are indexed [map][dir][y][x].

    walls int32[M, S], goal int32[M, 2]   the maps, as MerlinVecEnv.snapshot() gives them
    free   bool     the pose stands on no wall
    action int8     the policy's action, -1 where not free
    value  float32  the critic's value, NaN where not free
    steps  int16    actions until the policy's episode terminates, -1: never (merlin_policy_paths)
    dist   int16    the least number any behaviour needs, -1: none (merlin_shortest_paths' field)
    codes int32[n, 8], agent int32[n, 4], map_index int32[n] (optional): the free poses' views, in free_poses' order
    """
    size: int
    walls: torch.Tensor
    goal: torch.Tensor
    free: torch.Tensor
    action: torch.Tensor
    value: torch.Tensor
    steps: torch.Tensor
    dist: torch.Tensor
    codes: torch.Tensor | None = None
    agent: torch.Tensor | None = None
    map_index: torch.Tensor | None = None

    def at(self, agent: torch.Tensor):
        """(steps int64[M], dist int64[M]) at the poses agent int32[M, 4] = (x, y, dir, 0), pose m on map m; -1 for a
        pose outside the grid."""
        ok, idx = self._lookup(agent)
        none = torch.full((self.n_maps,), -1, dtype=torch.int64, device=ok.device)
        return torch.where(ok, self.steps[idx].long(), none), torch.where(ok, self.dist[idx].long(), none)

    def predicted_episode(self, agent: torch.Tensor, max_steps: int):
        """(reward float32[M], steps int64[M]) as evaluate_seeds reports the episode started in pose agent[m] of map
        m: where 1 <= steps <= max_steps the step kernel's reward at that step (merlin.pathing.optimal_reward's
        expression) after that many steps, otherwise (0.0, max_steps) -- the truncated episode."""
        ms = int(max_steps)
        st, _ = self.at(agent)
        solved = (st >= 1) & (st <= ms)
        return optimal_reward(st, ms), torch.where(solved, st, torch.full_like(st, ms))

    def optimal_actions(self) -> torch.Tensor:
        """bool[M, 4, S, S]: the pose's action terminates the episode, or leads to a pose whose dist is one less."""
        a, dist = self.action, self.dist.long()
        gx, gy = self.goal[:, 0].long(), self.goal[:, 1].long()
        S, M = self.size, self.n_maps
        is_goal = torch.zeros((M, S, S), dtype=torch.bool, device=dist.device)
        inside = (gx >= 0) & (gx < S) & (gy >= 0) & (gy < S)
        mi = torch.arange(M, device=dist.device)[inside]
        is_goal[mi, gy[inside], gx[inside]] = True
        front_goal = _front(is_goal.unsqueeze(1).expand(-1, 4, -1, -1).contiguous(), False)
        succ = torch.where(a == 0, dist.roll(1, dims=1),            # left: direction (d + 3) & 3 of the same cell
                           torch.where(a == 1, dist.roll(-1, dims=1),  # right: (d + 1) & 3
                                       torch.where(a == 2, _front(dist, -1), torch.full_like(dist, -1))))
        return self.free & (((a == 2) & front_goal) | ((succ >= 1) & (succ == dist - 1)))

    def metrics(self, max_steps: int, gamma: float = 0.99) -> dict:
        """Over the solvable poses (1 <= dist <= max_steps) of all maps pooled, in float64:
        solved_rate (1 <= steps <= max_steps), trapped_rate (steps == -1), timeout_rate (steps > max_steps), spl (mean
        of solved * dist / steps), excess_steps (mean of steps - dist over the solved poses), optimal_action_rate
        (optimal_actions), value_rmse (the critic against the greedy return from step 0: gamma^(steps - 1) * the
        reward at `steps` for a solved pose, 0 otherwise); n_maps, n_free, n_solvable; per_map: the same rates map by
        map (lists; nan for a map without a solvable pose).  With no solvable pose the means are nan."""
        ms = int(max_steps)
        f64 = torch.float64
        st, dist = self.steps.long(), self.dist.long()
        solvable = self.free & (dist >= 1) & (dist <= ms)
        solved = solvable & (st >= 1) & (st <= ms)
        trapped = solvable & (st == -1)
        timeout = solvable & (st > ms)
        spl = torch.where(solved, dist.to(f64) / st.clamp(min=1).to(f64), torch.zeros((), dtype=f64, device=st.device))
        excess = torch.where(solved, (st - dist).to(f64), torch.zeros((), dtype=f64, device=st.device))
        optimal = self.optimal_actions() & solvable
        ret = torch.where(solved, torch.pow(torch.tensor(float(gamma), dtype=f64, device=st.device),
                                            (st - 1).clamp(min=0).to(f64)) * optimal_reward(st, ms).to(f64),
                          torch.zeros((), dtype=f64, device=st.device))
        err2 = torch.where(solvable, (torch.nan_to_num(self.value.to(f64)) - ret) ** 2,
                           torch.zeros((), dtype=f64, device=st.device))

        named = {"solved_rate": (solved, solvable), "trapped_rate": (trapped, solvable),
                 "timeout_rate": (timeout, solvable), "spl": (spl, solvable), "excess_steps": (excess, solved),
                 "optimal_action_rate": (optimal, solvable)}
        out = {"n_maps": self.n_maps, "n_free": int(self.free.sum()), "n_solvable": int(solvable.sum()),
               "max_steps": ms, "gamma": float(gamma)}
        out.update({k: float(ratio(v, den)) for k, (v, den) in named.items()})
        out["value_rmse"] = float(ratio(err2, solvable)) ** 0.5
        out["per_map"] = {k: ratio(v, den, per_map=True).cpu().tolist() for k, (v, den) in named.items()}
        out["per_map"]["n_solvable"] = solvable.sum(dim=(1, 2, 3)).cpu().tolist()
        return out


def field_from_actions(walls: torch.Tensor, goal: torch.Tensor, action: torch.Tensor, value: torch.Tensor,
                       size: int, **extra) -> PolicyField:
    """The PolicyField of the action field action int8[M, 4, S, S] (and value float32 of that shape): steps and dist
    from the kernels for device tensors (merlin_policy_paths, merlin_shortest_paths), from the library's host
    restatements for CPU tensors."""
    S = int(size)
    free = free_cells(walls, S).unsqueeze(1).expand(-1, 4, -1, -1).contiguous()
    action = torch.where(free, action, torch.full_like(action, -1)).contiguous()
    if walls.is_cuda:
        steps = nat.policy_paths(walls, goal, action, S)
    else:
        steps = torch.from_numpy(nat.policy_paths_host(walls.numpy(), goal.numpy(), action.numpy(), S))
    return PolicyField(S, walls, goal, free, action, value, steps, distance_field(walls, goal, S), **extra)


@torch.no_grad()
def policy_field(ac, walls: torch.Tensor, goal: torch.Tensor, size: int, chunk: int = 65536) -> PolicyField:
    """The field of policy `ac` -- any object with act_codes(codes, deterministic=True) -> (action, logp, value) -- on
    the maps walls int32[M, S], goal int32[M, 2] (device tensors, MerlinVecEnv.snapshot()'s layouts): one view_codes
    launch over all free poses, the policy's forward in chunks of `chunk` frames, one policy_paths and one
    shortest_paths launch."""
    from .actor_critic import MLPActorCritic

    if isinstance(ac, MLPActorCritic) or not hasattr(ac, "act_codes"):
        raise ValueError("the policy field needs a policy that acts on the view codes (act_codes), "
                         f"got {type(ac).__name__}")
    def forward(codes):
        action, _, value = ac.act_codes(codes, deterministic=True)
        return action, value

    (action, value), codes, agent, index = over_free_poses(
        walls, goal, size, chunk, forward, ((torch.int8, (), -1), (torch.float32, (), float("nan"))))
    return field_from_actions(walls, goal, action, value, size, codes=codes, agent=agent, map_index=index)


def policy_field_for_seeds(ac, seeds, difficulty="mediumhard", size: int = 16, device="cuda",
                           max_steps: int | None = None):
    """(field, agent int32[n, 4], max_steps): the policy field on the maps evaluate_seeds plays for `seeds` (one
    seeded vector env, one reset, one snapshot; `difficulty`: one name, or one per seed), the start poses, and the
    effective episode limit.  field.predicted_episode(agent, max_steps) lines up with evaluate_seeds seed by seed."""
    walls, goal, agent, ms = maps_for_seeds(seeds, difficulty, size, device, max_steps)
    return policy_field(ac, walls, goal, size), agent, ms
