"""The numpy restatement of level mode (include/merlin_hip.h, "finite level sets and level replay"):
the level draw, the per-level scores and the replay weights, written from the contract and sharing no code with the
library or with merlin/levels.py.

draw     level of draw k of global env e = searchsorted(cdf, u, 'left') clipped to L - 1, u = the action draw's
         uniform01(level_seed, epoch 0, step k, env e, j 0) (tests/draw_ref.py)
scores   a step in level l in [0, L) adds rint(f * 2^24), f = fmin(|a| or fmax(a, 0), 32768) in float32, to sum[l] and
         1 to count[l]
weights  prioritized level replay with proportionate replay of unseen levels (see plr_weights)
"""
import numpy as np

import draw_ref as D

SCALE = 2.0 ** 24


def draw(level_seed, env, k, cdf):
    """int64 levels; `env` and `k` broadcast against each other."""
    cdf = np.asarray(cdf, dtype=np.float64)
    u = D.uniform01(level_seed, 0, np.asarray(k, dtype=np.uint64), np.asarray(env, dtype=np.uint64), 0)
    return np.minimum(np.searchsorted(cdf, u, side="left"), cdf.size - 1).astype(np.int64)


def draws(level_seed, env_first, n, k_first, k_count, cdf):
    """int64[n, k_count], merlin_level_draw_host's layout.  env_first may lie beyond 2^63 - 1: Python ints."""
    env = np.array([(int(env_first) + i) & D.M64 for i in range(n)], dtype=np.uint64)[:, None]
    k = np.array([(int(k_first) + j) & D.M64 for j in range(k_count)], dtype=np.uint64)[None, :]
    return draw(level_seed, env, k, cdf)


def step_scores(adv, kind):
    """int64, adv's shape: one step's addend."""
    a = np.asarray(adv, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        f = np.fmin(np.abs(a) if kind == 0 else np.fmax(a, np.float32(0.0)), np.float32(32768.0))
    assert f.dtype == np.float32
    return np.rint(f.astype(np.float64) * SCALE).astype(np.int64)


def scores(adv, levels, L, kind, sum0=None, count0=None):
    """(sum int64[L], count int64[L]); sum0 / count0: the vectors accumulated into."""
    s = np.zeros(L, dtype=np.int64) if sum0 is None else np.array(sum0, dtype=np.int64)
    c = np.zeros(L, dtype=np.int64) if count0 is None else np.array(count0, dtype=np.int64)
    lv = np.asarray(levels).reshape(-1).astype(np.int64)
    add = step_scores(adv, kind).reshape(-1)
    ok = (lv >= 0) & (lv < L)
    np.add.at(s, lv[ok], add[ok])
    np.add.at(c, lv[ok], 1)
    return s, c


def plr_weights(score, last_seen, seen, iteration, beta, rho):
    """float64[L] probabilities.  Seen levels ranked by score, descending, ties to the lower index; P_S ~ rank^(-1 /
    beta); P_C ~ iteration - last_seen, dropped when it sums to 0; P_seen = (1 - rho) P_S + rho P_C; the seen levels
    share |seen| / L of the mass as P_seen, each unseen level has 1 / L."""
    score = np.asarray(score, dtype=np.float64)
    seen = np.asarray(seen, dtype=bool)
    L = score.size
    p = np.full(L, 1.0 / L)
    idx = np.flatnonzero(seen)
    if idx.size == 0:
        return p
    order = idx[np.argsort(-score[idx], kind="stable")]
    rank = np.empty(idx.size)
    rank[np.searchsorted(idx, order)] = np.arange(1, idx.size + 1)
    ps = rank ** (-1.0 / beta)
    ps = ps / ps.sum()
    stale = (iteration - np.asarray(last_seen, dtype=np.int64)[idx]).astype(np.float64)
    pseen = (1.0 - rho) * ps + rho * stale / stale.sum() if stale.sum() > 0 else ps
    p[idx] = pseen * (idx.size / L)
    return p


def cdf_of(weights):
    c = np.cumsum(np.asarray(weights, dtype=np.float64))
    c[-1] = 1.0
    return c


class Sampler:
    """merlin.levels.LevelSampler's state machine on numpy arrays."""

    def __init__(self, L, strategy="plr", beta=0.1, rho=0.1):
        self.L, self.strategy, self.beta, self.rho = L, strategy, beta, rho
        self.score = np.zeros(L)
        self.last_seen = np.zeros(L, dtype=np.int64)
        self.seen = np.zeros(L, dtype=bool)
        self.iteration = 0

    def update(self, s, c, iteration):
        now = np.asarray(c) > 0
        self.score[now] = np.asarray(s, dtype=np.float64)[now] / np.asarray(c, dtype=np.float64)[now] / SCALE
        self.last_seen[now] = iteration
        self.seen |= now
        self.iteration = iteration

    def weights(self):
        if self.strategy == "uniform":
            return np.full(self.L, 1.0 / self.L)
        return plr_weights(self.score, self.last_seen, self.seen, self.iteration, self.beta, self.rho)

    def cdf(self):
        if self.strategy == "uniform":
            c = np.arange(1, self.L + 1, dtype=np.float64) / self.L
            c[-1] = 1.0
            return c
        return cdf_of(self.weights())


# advantages whose addend is worked out by hand in tests/test_level_host.py: +-0, NaN, +-inf, +-40000 (clamped), the
# clamp itself, values that round to 0, a rounding tie, its odd neighbour, +-0.5, and 1 + 2^-23
SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 40000.0, -40000.0, 32768.0, 1e-9, -1e-9, 2.0 ** -25,
                    3 * 2.0 ** -25, 0.5, -0.5, 1.0 + 2.0 ** -23], dtype=np.float32)


def score_case(T, N, L, seed):
    """(adv float32[T, N], levels int32[T, N]) for the score tests: normal advantages with SPECIAL planted at both
    ends; levels in runs along t as a rollout's are (an env changes level only now and then), level 1 never used
    where L > 1 (an unseen level), and the ids -1, L and L + 1 (skipped steps) planted in every column."""
    rs = np.random.RandomState(seed)
    adv = (rs.randn(T, N) * 2).astype(np.float32)
    flat = adv.reshape(-1)
    m = min(SPECIAL.size, flat.size)
    flat[:m] = SPECIAL[:m]
    flat[flat.size - m:] = SPECIAL[:m][::-1]
    lv = rs.randint(0, L, size=(T, N)).astype(np.int32)
    keep = rs.rand(T, N) < 0.6  # a step keeps the level of the step before it
    for t in range(1, T):
        lv[t] = np.where(keep[t], lv[t - 1], lv[t])
    lv[lv == 1] = 0
    cols = np.arange(N)
    for j, bad in enumerate((-1, L, L + 1)):
        rows = (cols + j) % T
        lv[rows, cols] = np.where(cols % 3 == j, bad, lv[rows, cols])
    assert (lv < 0).any() and (lv >= L).any() and (L == 1 or not (lv == 1).any())
    return adv, lv
