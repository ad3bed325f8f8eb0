"""The sampled-policy field: what a policy that SAMPLES its actions does from every pose of a map.

merlin/policy_field.py looks at the argmax policy; training, FOMAML's support rollouts and few-shot adaptation all act
by sampling.  The fact §6e rests on -- the view depends on (map, pose) only, the step count is not observed -- makes
the sampled case exact as well: the policy's probabilities turn a map into a time-homogeneous Markov chain over its
4 S^2 poses, and a dynamic programme over that chain and the horizon gives everything an episode's result is made of,
with no sampling noise and no episode played.

``sampled_field``             codes of all free poses (merlin._native.view_codes) -> the policy's probabilities and
                              value (``ac.probs_codes``) -> success / ret / steps / disc of every pose
                              (merlin._native.policy_chain) and the shortest-path field dist beside them.
``sampled_field_from_probs``  the same from a probability field: the kernels for device tensors, the library's host
                              restatements for CPU tensors.
``sampled_field_for_seeds``   on the maps evaluate_seeds plays for a list of seeds, with their start poses.
``SampledField``              ``at`` (the expected result of a sampled episode from one pose per map), ``occupancy``
                              (expected visits per pose and the episode-length distribution, forwards from a pose)
                              and ``metrics`` (over the solvable poses: success rate, expected return and steps, the
                              regret against the shortest path and the critic's error against the sampled return).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _native as nat
from .pathing import optimal_reward
from .pose_fields import PoseField, distance_field, free_cells, maps_for_seeds, over_free_poses, ratio


@dataclass
class SampledField(PoseField):
    """All tensors on one device; the [M, 4, S, S] fields are indexed [map][dir][y][x].

    walls int32[M, S], goal int32[M, 2]   the maps, as MerlinVecEnv.snapshot() gives them
    free    bool     the pose stands on no wall
    probs   float32[M, 4, S, S, 3]  the policy's probabilities (left, right, forward); 1/3 each where not free
    value   float32  the critic's value, NaN where not free
    success float64  P(an episode started here, sampled, reaches the goal within max_steps); NaN where not free
    ret     float64  its expected reward; steps float64: its expected length
    disc    float64  its expected discounted return from step 0: what the critic estimates
    dist    int16    the least number of actions any behaviour needs, -1: none (merlin_shortest_paths' field)
    """
    size: int
    max_steps: int
    gamma: float
    walls: torch.Tensor
    goal: torch.Tensor
    free: torch.Tensor
    probs: torch.Tensor
    value: torch.Tensor
    success: torch.Tensor
    ret: torch.Tensor
    steps: torch.Tensor
    disc: torch.Tensor
    dist: torch.Tensor

    def at(self, agent: torch.Tensor):
        """(success, ret, steps), float64[M]: the expected result of a sampled episode started in pose agent[m] =
        (x, y, dir, 0) of map m -- for the start poses of sampled_field_for_seeds, of the episode of seed m.  NaN for a
        pose outside the grid or on a wall."""
        ok, idx = self._lookup(agent)
        nan = torch.full((self.n_maps,), float("nan"), dtype=torch.float64, device=ok.device)
        return tuple(torch.where(ok, f[idx], nan) for f in (self.success, self.ret, self.steps))

    def occupancy(self, agent: torch.Tensor):
        """(visits float64[M, 4, S, S], hit float64[M, max_steps]) of the episode started in pose agent[m] of map m:
        the expected number of visits to every pose, and hit[m, t - 1] = P(the episode terminates at action t).
        visits.sum() over a map is `steps` at the start pose, hit.sum() is `success` there."""
        agent = agent.to(self.walls.device).to(torch.int32).contiguous()
        if agent.shape != (self.n_maps, 4):
            raise ValueError(f"one pose per map: expected {self.n_maps}x4, got {tuple(agent.shape)}")
        if self.walls.is_cuda:
            return nat.policy_occupancy(self.walls, self.goal, self.probs, agent, self.size, self.max_steps)
        v, h = nat.policy_occupancy_host(self.walls.numpy(), self.goal.numpy(), self.probs.numpy(), agent.numpy(),
                                         self.size, self.max_steps)
        return torch.from_numpy(v), torch.from_numpy(h)

    def metrics(self) -> dict:
        """Over the solvable poses (1 <= dist <= max_steps) of all maps pooled, in float64: success_rate (mean of
        success), expected_return (mean of ret), expected_steps (mean of steps), return_regret (mean of
        optimal_reward(dist) - ret) and value_rmse_sampled (the critic against disc); n_maps, n_free, n_solvable;
        per_map: the same map by map (lists; nan for a map without a solvable pose).  With no solvable pose the means
        are nan."""
        ms = self.max_steps
        f64 = torch.float64
        dist = self.dist.long()
        solvable = self.free & (dist >= 1) & (dist <= ms)
        zero = torch.zeros((), dtype=f64, device=dist.device)

        def on(v):
            return torch.where(solvable, v.to(f64), zero)

        named = {"success_rate": on(self.success), "expected_return": on(self.ret), "expected_steps": on(self.steps),
                 "return_regret": on(optimal_reward(dist, ms).to(f64) - self.ret)}
        err2 = on((torch.nan_to_num(self.value.to(f64)) - self.disc) ** 2)

        out = {"n_maps": self.n_maps, "n_free": int(self.free.sum()), "n_solvable": int(solvable.sum()),
               "max_steps": ms, "gamma": float(self.gamma)}
        out.update({k: float(ratio(v, solvable)) for k, v in named.items()})
        out["value_rmse_sampled"] = float(ratio(err2, solvable)) ** 0.5
        out["per_map"] = {k: ratio(v, solvable, per_map=True).cpu().tolist() for k, v in named.items()}
        out["per_map"]["value_rmse_sampled"] = ratio(err2, solvable, per_map=True).sqrt().cpu().tolist()
        out["per_map"]["n_solvable"] = solvable.sum(dim=(1, 2, 3)).cpu().tolist()
        return out


def sampled_field_from_probs(walls: torch.Tensor, goal: torch.Tensor, probs: torch.Tensor, value: torch.Tensor,
                             size: int, max_steps: int, gamma: float = 0.99) -> SampledField:
    """The SampledField of the probability field probs float32[M, 4, S, S, 3] (and value float32[M, 4, S, S]): the
    four chain fields and dist from the kernels for device tensors (merlin_policy_chain, merlin_shortest_paths), from
    the library's host restatements for CPU tensors.  A free pose whose row is negative, non-finite or sums to zero
    raises MerlinNativeError; wall poses' rows are replaced by 1/3 each."""
    S, T = int(size), int(max_steps)
    free = free_cells(walls, S).unsqueeze(1).expand(-1, 4, -1, -1).contiguous()
    probs = torch.where(free.unsqueeze(-1), probs.float(), torch.full_like(probs, 1.0 / 3.0, dtype=torch.float32))
    probs = probs.contiguous()
    value = torch.where(free, value.float(), torch.full_like(value, float("nan"), dtype=torch.float32))
    if walls.is_cuda:
        fields = nat.policy_chain(walls, goal, probs, S, T, gamma=gamma)
    else:
        fields = nat.policy_chain_host(walls.numpy(), goal.numpy(), probs.numpy(), S, T, gamma=gamma)
        fields = tuple(torch.from_numpy(f) for f in fields)
    return SampledField(S, T, float(gamma), walls, goal, free, probs, value, *fields, distance_field(walls, goal, S))


@torch.no_grad()
def sampled_field(ac, walls: torch.Tensor, goal: torch.Tensor, size: int, max_steps: int, gamma: float = 0.99,
                  chunk: int = 65536) -> SampledField:
    """The sampled field of policy `ac` -- any object with probs_codes(codes) -> (probs float32[n, 3], value [n]) --
    on the maps walls int32[M, S], goal int32[M, 2] (device tensors, MerlinVecEnv.snapshot()'s layouts): one
    view_codes launch over all free poses, the policy's forward in chunks of `chunk` frames, a scatter into the
    [M, 4, S, S] fields, one policy_chain and one shortest_paths launch."""
    from .actor_critic import MLPActorCritic

    if isinstance(ac, MLPActorCritic) or not hasattr(ac, "probs_codes"):
        raise ValueError("the sampled field needs a policy that gives probabilities on the view codes (probs_codes), "
                         f"got {type(ac).__name__}")
    (probs, value), *_ = over_free_poses(walls, goal, size, chunk, ac.probs_codes,
                                         ((torch.float32, (3,), 1.0 / 3.0), (torch.float32, (), float("nan"))))
    return sampled_field_from_probs(walls, goal, probs, value, size, max_steps, gamma)


def sampled_field_for_seeds(ac, seeds, difficulty="mediumhard", size: int = 16, device="cuda",
                            max_steps: int | None = None, gamma: float = 0.99):
    """(field, agent int32[n, 4], max_steps): the sampled field on the maps evaluate_seeds plays for `seeds` (one
    seeded vector env, one reset, one snapshot; `difficulty`: one name, or one per seed), the start poses, and the
    effective episode limit.  field.at(agent) is the expected result of a sampled episode of each seed."""
    walls, goal, agent, ms = maps_for_seeds(seeds, difficulty, size, device, max_steps)
    return sampled_field(ac, walls, goal, size, ms, gamma=gamma), agent, ms
