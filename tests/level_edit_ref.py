"""The level-editing tests' own reference (no test in here): a numpy / plain-Python restatement of the edit rule written
from its contract (include/merlin_hip.h, "level editing"), on draw_ref.uniform01 and pathing_ref.bfs.  It shares no
code with the library.

Child c of generation g is its parent after E edits e = 0 .. E - 1; u_j = uniform01(seed, g, e, c, j), j = 0, 1, 2;
kind = min(floor(4 u_0), 3); n = min(floor(u_1 (S-2)^2), (S-2)^2 - 1); cell (1 + n % (S-2), 1 + n / (S-2)); kind 0, 1
toggle the wall unless the cell is the agent's or the goal's; kind 2 moves the goal unless the cell is a wall, the
agent's or the goal's own; kind 3 moves the agent, dir = min(floor(4 u_2), 3), unless the cell is a wall or the goal's.

The hand-made maps: the open room, and the serpentine -- a full wall row at each even y in 2 .. S - 2, the k-th of them
with one gap, at x = 1 for even k and x = S - 2 for odd k; agent (1, 1, 0); goal (S - 2, S - 2), or (S - 2, S - 3) where
that cell is a wall.  On the serpentine an edit often lands on a wall row (goal and agent moves do nothing), and a wall
toggled into a corridor or a gap cuts the only path: every outcome class occurs among a few dozen children.
"""
import numpy as np

from draw_ref import uniform01
from pathing_ref import bfs

SIZES = (5, 7, 16, 22, 32)
EDIT_SEED, GENERATION, CHILDREN = 7, 1, 64  # the key of the recorded outcome counts below


def open_room(S):
    """(walls uint32[S], goal (x, y), agent (x, y, dir)): only the border is walled."""
    full, edge = (1 << S) - 1, 1 | (1 << (S - 1))
    w = np.full(S, edge, dtype=np.uint32)
    w[0] = w[S - 1] = full
    return w, (S - 2, S - 2), (1, 1, 0)


def serpentine(S):
    w, _, agent = open_room(S)
    full = (1 << S) - 1
    for k, y in enumerate(range(2, S - 1, 2)):
        gap = 1 if k % 2 == 0 else S - 2
        w[y] = full & ~(1 << gap)
    gx, gy = S - 2, S - 2
    if (int(w[gy]) >> gx) & 1:
        gy = S - 3
    assert not (int(w[gy]) >> gx) & 1
    return w, (gx, gy), agent


def bank(maps):
    """[(walls, goal, agent)] -> (walls uint32[P, S], goal int32[P, 2], agent int32[P, 4])."""
    walls = np.stack([m[0] for m in maps]).astype(np.uint32)
    goal = np.array([m[1] for m in maps], dtype=np.int32).reshape(-1, 2)
    agent = np.zeros((len(maps), 4), dtype=np.int32)
    agent[:, :3] = np.array([m[2] for m in maps], dtype=np.int32).reshape(-1, 3)
    return walls, goal, agent


def cells_of(w, S):
    return ((np.asarray(w, dtype=np.uint64)[:, None] >> np.arange(S, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def solve(w, goal, agent, S):
    return bfs(cells_of(w, S), (agent[0], agent[1]), agent[2], goal)


def mutate(walls, goal, agent, parent_index, C, S, edits, seed, generation):
    """The rule on a bank: (walls uint32[C, S], goal int32[C, 2], agent int32[C, 4], dist int32[C], changed uint8[C],
    noop int64[C, 3]) -- noop[c, k]: edits of child c that did nothing, by class (0: a toggle, 1: a goal move, 2: an
    agent move).  parent_index None: child c edits parent c.  A parent outside the bank: zeros, dist -1, changed 0."""
    P = walls.shape[0]
    ow = np.zeros((C, S), dtype=np.uint32)
    og = np.zeros((C, 2), dtype=np.int32)
    oa = np.zeros((C, 4), dtype=np.int32)
    dist = np.full(C, -1, dtype=np.int32)
    changed = np.zeros(C, dtype=np.uint8)
    noop = np.zeros((C, 3), dtype=np.int64)
    side = S - 2
    cells = side * side
    for c in range(C):
        p = c if parent_index is None else int(parent_index[c])
        if not 0 <= p < P:
            continue
        w = [int(v) for v in walls[p]]
        gx, gy = (int(v) for v in goal[p])
        ax, ay, d, a3 = (int(v) for v in agent[p])
        for e in range(edits):
            u = [float(uniform01(seed, generation, e, c, j)) for j in range(3)]
            kind = min(int(np.floor(u[0] * 4.0)), 3)
            n = min(int(np.floor(u[1] * float(cells))), cells - 1)
            x, y = 1 + n % side, 1 + n // side
            wall = (w[y] >> x) & 1
            at_agent, at_goal = (x, y) == (ax, ay), (x, y) == (gx, gy)
            if kind <= 1:
                if at_agent or at_goal:
                    noop[c, 0] += 1
                else:
                    w[y] ^= 1 << x
            elif kind == 2:
                if wall or at_agent or at_goal:
                    noop[c, 1] += 1
                else:
                    gx, gy = x, y
            else:
                if wall or at_goal:
                    noop[c, 2] += 1
                else:
                    ax, ay, d = x, y, min(int(np.floor(u[2] * 4.0)), 3)
        ow[c], og[c], oa[c] = w, (gx, gy), (ax, ay, d, a3)
        changed[c] = int((ow[c] != walls[p]).any() or (og[c] != goal[p]).any() or (oa[c] != agent[p]).any())
        dist[c] = solve(ow[c], (gx, gy), (ax, ay, d), S)
    return ow, og, oa, dist, changed, noop


def outcome(maker, S, edits, C=CHILDREN, seed=EDIT_SEED, generation=GENERATION):
    """The children of one hand-made map under the recorded key: mutate()'s tuple, every child from parent 0."""
    walls, goal, agent = bank([maker(S)])
    return mutate(walls, goal, agent, np.zeros(C, dtype=np.int32), C, S, edits, seed, generation)


# ---- the selection logic of merlin.level_edit, restated with Python lists ------------------------------------------
def parents_ref(score, seen, C):
    """[(level, is a seen level)] of the C best: seen levels by score descending, ties to the lower index, then the
    unseen ones by index."""
    L = len(score)
    order = sorted(range(L), key=lambda l: (0, -score[l], l) if seen[l] else (1, 0.0, l))
    return [(l, bool(seen[l])) for l in order[:C]]


def victims_ref(weights, seen, parents, C):
    """The C seen non-parent levels of lowest weight, ties to the lower index, padded with -1."""
    par = {l for l, ok in parents if ok}
    el = sorted((l for l in range(len(weights)) if seen[l] and l not in par), key=lambda l: (weights[l], l))
    el = el[:C]
    return el + [-1] * (C - len(el))
