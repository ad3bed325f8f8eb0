"""The policy-field tests' own reference (no test in here).  It shares nothing with the library: `walk` applies the
step rule forwards, action by action, from every pose -- the kernel searches backwards from the goal in layers, the
library's host restatement walks with memoisation and cycle marks; this one does neither and simply stops counting.

The step rule: 0 turn left (dir + 3) & 3, 1 turn right (dir + 1) & 3, 2 forward into a non-wall cell, terminating on
the forward action whose front cell is the goal; directions 0 = +x, 1 = +y, 2 = -x, 3 = -y.  Fields are indexed
[dir][y][x]; cells[y][x] == 1 is a wall (oracle.gen_map)."""
import numpy as np
import torch

from pathing_ref import CASES, IDS, oracle_maps  # noqa: F401

DX, DY = np.array([1, 0, -1, 0]), np.array([0, 1, 0, -1])
SEEDS9 = list(range(1000, 1009))


def successors(cells, goal, action_field):
    """int64[P + 2] for one map, P = 4 S^2 poses numbered (d * S + y) * S + x: the pose after the pose's own action;
    P = the episode has terminated, P + 1 = it never will (a wall pose, an action outside {0, 1, 2}, a forward move
    into a wall or off the grid).  Both are absorbing."""
    S = cells.shape[0]
    P = 4 * S * S
    d, y, x = np.meshgrid(np.arange(4), np.arange(S), np.arange(S), indexing="ij")
    a = np.asarray(action_field).astype(np.int64)
    wall = cells == 1
    fx, fy = x + DX[d], y + DY[d]
    inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
    fxc, fyc = np.clip(fx, 0, S - 1), np.clip(fy, 0, S - 1)
    blocked = ~inside | wall[fyc, fxc]
    at_goal = inside & (fx == int(goal[0])) & (fy == int(goal[1]))
    pose = lambda dd, yy, xx: (dd * S + yy) * S + xx  # noqa: E731
    nxt = np.full((4, S, S), P + 1, dtype=np.int64)
    nxt = np.where(a == 0, pose((d + 3) & 3, y, x), nxt)
    nxt = np.where(a == 1, pose((d + 1) & 3, y, x), nxt)
    nxt = np.where((a == 2) & ~blocked, np.where(at_goal, P, pose(d, fyc, fxc)), nxt)
    nxt = np.where(wall[y, x], P + 1, nxt)
    return np.concatenate([nxt.reshape(-1), [P, P + 1]])


def walk(cells, goal, action_field):
    """int16[4, S, S] (or [M, 4, S, S] for stacked maps): from every pose, the step rule applied pose by pose for at
    most 4 S^2 + 1 actions; the number of actions at which the episode terminated, -1 if it has not by then."""
    cells, goal, action_field = np.asarray(cells), np.asarray(goal), np.asarray(action_field)
    if cells.ndim == 2:
        return walk(cells[None], goal[None], action_field[None])[0]
    M, S = cells.shape[0], cells.shape[1]
    P = 4 * S * S
    # all maps in one table: map m's poses and its two absorbing states at m * (P + 2)
    succ = np.concatenate([successors(cells[m], goal[m], action_field[m]) + m * (P + 2) for m in range(M)])
    term = (np.arange(M) * (P + 2) + P)[:, None]
    cur = (np.arange(M)[:, None] * (P + 2) + np.arange(P)[None, :])
    res = np.full((M, P), -1, dtype=np.int64)
    for t in range(1, P + 2):
        cur = succ[cur]
        res[(cur == term) & (res < 0)] = t
        if not ((cur - term) < 0).any():  # nobody is still walking
            break
    return res.reshape(M, 4, S, S).astype(np.int16)


# -- action fields written from the cells ---------------------------------------------------------------------------
def bouncer_field(cells):
    """int8[4, S, S]: forward unless the front cell is a wall or off the grid, then turn right -- what Bouncer sees
    (the front cell is view cell (3, 5), always lit; the view shows cells off the grid as walls)."""
    S = cells.shape[0]
    d, y, x = np.meshgrid(np.arange(4), np.arange(S), np.arange(S), indexing="ij")
    fx, fy = x + DX[d], y + DY[d]
    inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
    blocked = ~inside | (cells[np.clip(fy, 0, S - 1), np.clip(fx, 0, S - 1)] == 1)
    return np.where(blocked, 1, 2).astype(np.int8)


def seeker_field(cells, goal):
    """int8[4, S, S]: forward if the goal lies 1..6 cells straight ahead with no wall before it (view column 3 is lit
    up to its first wall), else turn left -- what Seeker sees."""
    S = cells.shape[0]
    d, y, x = np.meshgrid(np.arange(4), np.arange(S), np.arange(S), indexing="ij")
    seen = np.zeros((4, S, S), dtype=bool)
    clear = np.ones((4, S, S), dtype=bool)
    for k in range(1, 7):
        fx, fy = x + k * DX[d], y + k * DY[d]
        inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
        wall = ~inside | (cells[np.clip(fy, 0, S - 1), np.clip(fx, 0, S - 1)] == 1)
        clear &= ~wall
        seen |= clear & (fx == int(goal[0])) & (fy == int(goal[1]))
    return np.where(seen, 2, 0).astype(np.int8)


# -- scripted policies on the view codes: act_codes(codes int32[n, 8]) -> (action int64, logp f32, value f32) -------
def tile(codes: torch.Tensor, vi: int, vj: int) -> torch.Tensor:
    """The tile class (0 unseen, 1 empty, 2 wall, 3 goal, 4 agent) of view cell (vi, vj): nibble vj * 7 + vi."""
    k = vj * 7 + vi
    return (codes[:, k >> 3].long() >> ((k & 7) * 4)) & 0xF


class _Scripted:
    def act_codes(self, codes, deterministic=True, index=None):
        assert deterministic and index is None
        a = self.action(codes).long()
        z = torch.zeros(a.shape, dtype=torch.float32, device=codes.device)
        return a, z, z.clone()


class AlwaysLeft(_Scripted):
    def action(self, codes):
        return torch.zeros(codes.shape[0], dtype=torch.int64, device=codes.device)


class Bouncer(_Scripted):
    """Forward if view cell (3, 5) -- the cell in front -- is not a wall tile, else turn right."""

    def action(self, codes):
        return torch.where(tile(codes, 3, 5) == 2, 1, 2)


class Seeker(_Scripted):
    """Forward if any cell of view column 3 shows the goal tile and no wall lies before it, else turn left."""

    def action(self, codes):
        n = codes.shape[0]
        clear = torch.ones(n, dtype=torch.bool, device=codes.device)
        seen = torch.zeros(n, dtype=torch.bool, device=codes.device)
        for vj in range(5, -1, -1):  # from the cell in front outwards
            t = tile(codes, 3, vj)
            clear &= t != 2
            seen |= clear & (t == 3)
        return torch.where(seen, 2, 0)
