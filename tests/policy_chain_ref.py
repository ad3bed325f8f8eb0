"""The sampled-policy tests' own reference (no test in here): vectorised float64 numpy forms of the two recursions of
DESIGN.md §6f, written from the step rule in tests/policy_field_ref.py's docstring -- 0 turn left (dir + 3) & 3, 1 turn
right (dir + 1) & 3, 2 forward into a non-wall cell, terminating on the forward action whose front cell is the goal, a
forward move into a wall or off the grid leaving the pose where it is -- with the reward 1 - 0.9 t / T at action t and
truncation after T actions.  It shares nothing with the library: whole-array shifts over [M, 4, S, S] fields, where
the kernels gather per cell through LDS and the library's host restatements walk a successor table.

Fields are indexed [map][dir][y][x]; cells[m][y][x] == 1 is a wall; probs[..., a] is the probability of action a."""
import numpy as np

DX, DY = np.array([1, 0, -1, 0]), np.array([0, 1, 0, -1])


def normalise(probs):
    """float64 q_a = p_a / ((p_0 + p_1) + p_2): float32 softmax rows do not sum to 1."""
    p = np.asarray(probs).astype(np.float64)
    return p / ((p[..., 0] + p[..., 1]) + p[..., 2])[..., None]


def geometry(cells, goal):
    """bool[M, 4, S, S] each: free (the pose stands on no wall), front_goal (its front cell is the goal), blocked
    (its front cell is a wall or off the grid, and not the goal)."""
    cells, goal = np.asarray(cells), np.asarray(goal)
    M, S = cells.shape[0], cells.shape[1]
    d, y, x = np.meshgrid(np.arange(4), np.arange(S), np.arange(S), indexing="ij")
    fx, fy = x + DX[d], y + DY[d]
    inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
    wall = cells == 1
    fwall = wall[:, np.clip(fy, 0, S - 1), np.clip(fx, 0, S - 1)]
    gx, gy = goal[:, 0][:, None, None, None], goal[:, 1][:, None, None, None]
    front_goal = inside[None] & (fx[None] == gx) & (fy[None] == gy)
    blocked = ~front_goal & (~inside[None] | fwall)
    free = np.broadcast_to(~wall[:, None], (M, 4, S, S))
    return free, front_goal, blocked


def front(h):
    """h[M, 4, S, S] read at each pose's front pose (same direction); 0 where that is off the grid."""
    out = np.zeros_like(h)
    out[:, 0, :, :-1] = h[:, 0, :, 1:]
    out[:, 1, :-1, :] = h[:, 1, 1:, :]
    out[:, 2, :, 1:] = h[:, 2, :, :-1]
    out[:, 3, 1:, :] = h[:, 3, :-1, :]
    return out


def push(f):
    """f[M, 4, S, S] moved from each pose to its front pose (the inverse shift of `front`)."""
    out = np.zeros_like(f)
    out[:, 0, :, 1:] = f[:, 0, :, :-1]
    out[:, 1, 1:, :] = f[:, 1, :-1, :]
    out[:, 2, :, :-1] = f[:, 2, :, 1:]
    out[:, 3, :-1, :] = f[:, 3, 1:, :]
    return out


def reward(t, T):
    return 1.0 - 0.9 * (float(t) / float(T))


def chain_ref(cells, goal, probs, T, gamma=0.99):
    """dict of float64[M, 4, S, S]: success, ret, steps, disc; NaN at wall poses."""
    free, front_goal, blocked = geometry(cells, goal)
    q = np.where(free[..., None], normalise(probs), 0.0)
    qL, qR, qF = q[..., 0], q[..., 1], q[..., 2]
    h = np.where(front_goal, qF, 0.0)
    acc = {k: np.zeros_like(h) for k in ("success", "ret", "n", "disc")}
    g = 1.0
    for t in range(1, int(T) + 1):
        r = reward(t, T)
        acc["success"] += h
        acc["ret"] += h * r
        acc["n"] += t * h
        acc["disc"] += h * (g * r)
        g *= gamma
        ahead = np.where(front_goal, 0.0, np.where(blocked, h, front(h)))
        # left of direction d is (d + 3) & 3 = d - 1: np.roll(h, 1)[d] = h[d - 1]
        h = (qL * np.roll(h, 1, axis=1) + qR * np.roll(h, -1, axis=1)) + qF * ahead
    out = {"success": acc["success"], "ret": acc["ret"], "steps": acc["n"] + T * (1.0 - acc["success"]),
           "disc": acc["disc"]}
    return {k: np.where(free, v, np.nan) for k, v in out.items()}


def occupancy_ref(cells, goal, probs, agent, T):
    """(visits float64[M, 4, S, S], hit float64[M, T]) from the start poses agent int32[M, 4] = (x, y, dir, 0), all
    of them free poses of the grid."""
    free, front_goal, blocked = geometry(cells, goal)
    q = np.where(free[..., None], normalise(probs), 0.0)
    qL, qR, qF = q[..., 0], q[..., 1], q[..., 2]
    M = free.shape[0]
    mu = np.zeros(free.shape, dtype=np.float64)
    mu[np.arange(M), agent[:, 2], agent[:, 1], agent[:, 0]] = 1.0
    assert (mu[~free] == 0).all()
    visits = np.zeros_like(mu)
    hit = np.zeros((M, int(T)), dtype=np.float64)
    for t in range(int(T)):
        visits += mu
        f = qF * mu
        per_dir = np.where(front_goal, f, 0.0).sum(axis=(2, 3))
        hit[:, t] = ((per_dir[:, 0] + per_dir[:, 1]) + per_dir[:, 2]) + per_dir[:, 3]
        moving = np.where(front_goal | blocked, 0.0, f)
        # a left turn takes direction d to d - 1: the mass arriving in d comes from d + 1
        mu = (np.roll(qL * mu, -1, axis=1) + np.roll(qR * mu, 1, axis=1)) + push(moving) + np.where(blocked, f, 0.0)
    return visits, hit


def corridor_closed_form(q, T):
    """A free cell beside the goal on which the pose facing the goal goes forward with probability q and turns left
    with 1 - q, and the other three poses turn left with probability 1: the pose that needs j left turns to face the
    goal (j = 0: the facing pose) terminates at action j + 1 + 4 k with probability q (1 - q)^k, k = 0, 1, ..., as
    long as that action is within T.  -> (success, ret, steps) float64[4], indexed by j."""
    out = np.zeros((3, 4), dtype=np.float64)
    for j in range(4):
        s = r = n = 0.0
        k = 0
        while j + 1 + 4 * k <= T:
            t = j + 1 + 4 * k
            p = q * (1.0 - q) ** k
            s += p
            r += p * reward(t, T)
            n += p * t
            k += 1
        out[:, j] = (s, r, n + T * (1.0 - s))
    return out


def dirichlet_field(m, size, seed):
    """float32[m, 4, size, size, 3]: a seeded Dirichlet(1, 1, 1) row per pose, cast to float32 (rows no longer sum
    to 1 exactly)."""
    return np.random.RandomState(seed).dirichlet((1.0, 1.0, 1.0), size=(m, 4, size, size)).astype(np.float32)


def one_hot(action):
    """float32[..., 3] of an action field with values in {0, 1, 2}."""
    a = np.asarray(action)
    assert ((a >= 0) & (a <= 2)).all()
    return (a[..., None] == np.arange(3)).astype(np.float32)
