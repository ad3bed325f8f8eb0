"""Level editing: the level bank evolves by mutation (ACCEL, Parker-Holder et al. 2022).

``mutate_levels``  children of chosen parents of a LevelSet: a few random edits each (toggle a wall, move the goal, move
                   the agent), with each child's shortest-path length and whether it differs from its parent -- one HIP
                   kernel (merlin_levels_mutate), no host sync.
``LevelEditor``    one editing round on a bank under prioritized level replay: the highest-scoring seen levels are the
                   parents, a child that changed and is solvable takes the slot of a level the sampler weighs least, in
                   place in the env's bank (MerlinVecEnv.replace_levels), in the LevelSet and, as an unseen level, in the
                   sampler.  Selection is by replacement: a child is played soon (an unseen level has weight 1 / L),
                   scored by the rollout that plays it, and one the policy learns nothing from is a later round's victim.

merlin.PPO(level_editor=...) runs a round inside its update; ppo_train.py --level_replay accel wires it up.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .levels import LevelSet


def mutate_levels(level_set: LevelSet, parent_index, edits: int, seed: int, generation: int):
    """(children: LevelSet, dist int32[C], changed uint8[C]), device tensors: child c is level parent_index[c] (int32[C]
    on the set's device; None: level c) after `edits` edits keyed (seed, generation, edit, c) -- the rule of
    include/merlin_hip.h.  dist: the child's optimal step count, -1 if its goal cannot be reached.  An index outside
    the set gives an all-zero child, dist -1, changed 0."""
    walls, goal, agent, dist, changed = nat.levels_mutate(level_set.walls, level_set.goal, level_set.agent,
                                                          parent_index, level_set.size, edits, seed, generation)
    return LevelSet(walls, goal, agent, level_set.size), dist, changed


def select_parents(sampler, children: int):
    """(parents int64[C], ok bool[C]): the C seen levels of highest score, descending, ties to the lower index; the
    unseen levels rank behind every seen one and ok marks the entries that are seen levels.  Any device, no host sync."""
    key = torch.where(sampler.seen, sampler.score, torch.full_like(sampler.score, -float("inf")))
    parents = torch.sort(key, descending=True, stable=True).indices[:children]
    return parents, sampler.seen[parents]


def select_victims(sampler, parents: torch.Tensor, parents_ok: torch.Tensor, children: int) -> torch.Tensor:
    """int64[C]: the C levels of lowest sampler.weights() among the seen levels that are not this round's parents,
    ascending, ties to the lower index; -1 where there are fewer such levels than children."""
    L = sampler.L
    is_parent = torch.zeros(L + 1, dtype=torch.bool, device=parents.device)
    is_parent[torch.where(parents_ok, parents, torch.full_like(parents, L))] = True
    eligible = sampler.seen & ~is_parent[:L]
    w = sampler.weights()
    key = torch.where(eligible, w, torch.full_like(w, float("inf")))
    order = torch.sort(key, descending=False, stable=True).indices[:children]
    return torch.where(eligible[order], order, torch.full_like(order, -1))


class LevelEditor:
    """children: children per round (at most L); edits: edits per child (0..64); min_dist: a child is accepted iff it
    changed and its optimal step count is at least min_dist (1: solvable); every: PPO runs a round every `every`-th
    update; seed: the edit key's seed.  The key holds no rank, and the scores a round reads are all-reduced: every
    rank of a data-parallel run builds the same bank.  accepted / rejected_unsolvable / rejected_unchanged: running
    device counters (int64[1]); last_accepted: the last round's."""

    def __init__(self, children: int, edits: int = 4, min_dist: int = 1, every: int = 1, seed: int = 0):
        if int(children) < 1:
            raise ValueError("LevelEditor: at least one child per round")
        if not 0 <= int(edits) <= nat.MAX_LEVEL_EDITS:
            raise ValueError(f"LevelEditor: edits in 0..{nat.MAX_LEVEL_EDITS}")
        if int(every) < 1:
            raise ValueError("LevelEditor: every >= 1")
        self.children, self.edits, self.min_dist = int(children), int(edits), int(min_dist)
        self.every, self.seed = int(every), int(seed)
        self.generation = 0  # rounds run so far: round g's edit key and its children's lineage carry g
        self.accepted = self.rejected_unsolvable = self.rejected_unchanged = self.last_accepted = None
        self.last_slots = self.last_parents = None

    def due(self, iteration: int) -> bool:
        return int(iteration) % self.every == 0

    def evolve(self, level_set: LevelSet, sampler, env, iteration: int) -> torch.Tensor:
        """One round, no host sync; returns the slots int32[C] the children took (-1: dropped).  `sampler` is the
        'plr' LevelSampler of the set (already updated with this iteration's scores), `env` the MerlinVecEnv the set is
        bound to (None: the set and the sampler alone)."""
        L = len(level_set)
        Cn = min(self.children, L)
        dev = level_set.device
        if self.accepted is None:
            self.accepted, self.rejected_unsolvable, self.rejected_unchanged, self.last_accepted = (
                torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(4))
        self.generation += 1
        parents, ok = select_parents(sampler, Cn)
        pidx = torch.where(ok, parents, torch.full_like(parents, -1)).to(torch.int32)
        kids, dist, changed = mutate_levels(level_set, pidx, self.edits, self.seed, self.generation)
        changed = changed != 0
        solvable = dist >= self.min_dist
        accept = ok & changed & solvable
        victims = select_victims(sampler, parents, ok, Cn)
        slots = torch.where(accept, victims, torch.full_like(victims, -1)).to(torch.int32)
        if env is not None:
            env.replace_levels(slots, kids)
        level_set.replace_(slots, kids, self.generation, pidx)
        sampler.forget(slots)
        self.last_accepted = (slots >= 0).sum().reshape(1)
        self.accepted = self.accepted + self.last_accepted
        self.rejected_unchanged = self.rejected_unchanged + (ok & ~changed).sum()
        self.rejected_unsolvable = self.rejected_unsolvable + (ok & changed & ~solvable).sum()
        self.last_slots, self.last_parents = slots, pidx
        return slots
