"""The draw tests' own reference (no test in here): a numpy restatement of the acting draw's contract (DESIGN.md §2;
act_finish / uniform01 in csrc/merlin_internal.h), and the fixed case list that tests/test_gpu_draw.py runs on the
device and tests/test_draw_ref.py vets on the CPU.

The contract: u_j = ((h_j >> 11) + 1) * 2^-53 with h_j four chained splitmix64 finalisers over (seed, epoch, step,
global env index, j); score_j = logp_j - log(-log u_j) in float64; the action is the first maximum.  The hash is
defined bit for bit, the decision up to the margin between the two best scores (`gap`), which is returned so that a
comparison can excuse the decisions the fp32 log-softmax of the device may turn."""
import math

import numpy as np

M64 = (1 << 64) - 1
# the key's constants (csrc/merlin_internal.h uniform01): the golden-ratio increment of splitmix64 added to the seed,
# an offset for the epoch, and odd multipliers that spread step and env over the word before the next finaliser
K_SEED, K_EPOCH, K_STEP, K_ENV = 0x9e3779b97f4a7c15, 0x632be59bd9b4e019, 0x8cb92ba72f3d8dd7, 0xd6e8feb86659fd93


def _u64(x):
    """Python ints (any sign, any size) or integer arrays -> uint64, modulo 2^64."""
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & M64)
    x = np.asarray(x)
    if x.dtype == np.uint64:
        return x
    if x.dtype == object:
        return np.array([int(v) & M64 for v in x.ravel()], dtype=np.uint64).reshape(x.shape)
    return x.astype(np.int64).astype(np.uint64)  # two's complement: the value modulo 2^64


def mix64(x):
    """The splitmix64 finaliser."""
    x = _u64(x)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))


def hash64(seed, epoch, step, env, j):
    """The 64 hash bits of one stream: the arguments broadcast against each other."""
    with np.errstate(over="ignore"):
        x = mix64(_u64(seed) + np.uint64(K_SEED))
        x = mix64(x ^ (_u64(epoch) + np.uint64(K_EPOCH)))
        x = mix64(x ^ (_u64(step) * np.uint64(K_STEP)))
        return mix64(x ^ (_u64(env) * np.uint64(K_ENV) + _u64(j)))


def bits_to_uniform(h):
    """((h >> 11) + 1) * 2^-53: in (0, 1], every step exact in float64."""
    return ((_u64(h) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def uniform01(seed, epoch, step, env, j):
    return bits_to_uniform(hash64(seed, epoch, step, env, j))


def log_softmax64(logits):
    z = np.asarray(logits, dtype=np.float64)
    z = z - z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def race(logp, u):
    """(first-maximum action, gap between the two best scores; inf when A = 1) of logp_j - log(-log u_j)."""
    with np.errstate(divide="ignore"):
        score = logp - np.log(-np.log(u))
    action = score.argmax(-1)  # numpy's argmax returns the first maximum
    if score.shape[-1] == 1:
        return action, np.full(action.shape, np.inf)
    with np.errstate(invalid="ignore"):  # inf - inf where two streams both drew u = 1
        top = np.sort(score, -1)
        gap = top[..., -1] - top[..., -2]
    return action, np.where(np.isnan(gap), 0.0, gap)


def expected_draw(logits64, seed, epoch, step, env):
    """logits64 f64[n, A] (or [A], shared by every env), env the global env indices [n] -> (float64 log-softmax
    [n, A], action [n], gap [n])."""
    env = np.atleast_1d(_u64(env))
    logp = log_softmax64(logits64)
    logp = np.broadcast_to(logp, (env.shape[0], logp.shape[-1]))
    u = uniform01(seed, epoch, step, env[:, None], np.arange(logp.shape[-1])[None, :])
    action, gap = race(logp, u)
    return logp, action, gap


# ------------------------------------------------------------------------------------------------------------------
# chi-square upper quantiles without a statistics package: the survival function in closed form (even df: a Poisson
# sum; odd df: erfc plus a half-integer sum), inverted by bisection
def chi2_sf(x, df):
    h = 0.5 * x
    if df % 2 == 0:
        term, s = 1.0, 1.0
        for k in range(1, df // 2):
            term *= h / k
            s += term
        return math.exp(-h) * s
    s, term = 0.0, math.sqrt(h) / math.gamma(1.5)  # h^(k - 1/2) / Gamma(k + 1/2) at k = 1
    for k in range(1, (df - 1) // 2 + 1):
        s += term
        term *= h / (k + 0.5)
    return math.erfc(math.sqrt(h)) + math.exp(-h) * s


def chi2_upper(df, q=1e-6):
    """x with P(chi2_df > x) = q."""
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf(mid, df) > q else (lo, mid)
    return 0.5 * (lo + hi)


# ------------------------------------------------------------------------------------------------------------------
# The device cases.  Logits are multiples of 2^-10 in [-8, 8] (spread <= 16): exact in fp32, and so are their sums with
# the shift that carries them through act_heads' ReLU and with the biases, so the device's logits are the host's and
# only its fp32 log-softmax rounds.  MARGIN is derived, not measured: the device scores (double)float(z_j - lse), the
# lse's own error is common to every j, which leaves one fp32 rounding of a value below 32 per score (<= 2^-20 each,
# 1.9e-6 for the pair) plus float64 log ulps.
MARGIN = 1e-5
EXCUSED_CAP = 1e-4     # largest share of a case's decisions under the margin
EXACT_BELOW = 10_000   # cases with fewer decisions hold none under the margin at all
LOGP_ATOL = 1e-5       # tests/test_gpu_act.py's atol for the same quantity
SHIFT = 16.0           # act_heads: z = logit + SHIFT - bias > 0

BALANCED = (0.5, 0.3, 0.2)
SKEW3 = (0.97, 0.025, 0.005)
SKEW4 = (0.6, 0.3, 0.0999, 0.0001)
SKEW2 = (0.999, 0.001)
DECADES8 = (0.45, 0.25, 0.15, 0.08, 0.04, 0.02, 0.0095, 0.0005)  # three decades
NEAR_UNIFORM = (0.34, 0.33, 0.33)


def _case(entry, n, A, width, seed, epoch, step, env_offset, dist, bias, lseed):
    return dict(entry=entry, n=n, A=A, width=width, seed=seed, epoch=epoch, step=step, env_offset=env_offset,
                dist=dist, bias=bias, lseed=lseed, margin=MARGIN,
                id=f"{entry}-n{n}-A{A}-w{width}-{dist if isinstance(dist, str) else 'p%g' % dist[0]}")


# entry, n, A, P (draw) or H (heads), seed, epoch, step, env_offset, distribution, biases, seed of the logits.
# Every value of the issue's lists appears once; each entry point has the balanced case that the power test of
# tests/test_draw_ref.py shows is needed, skewed ones and per-env random logits.
CASES = [
    _case("draw", 1, 1, 1, 0, 0, 0, 0, "random", "zero", 101),
    _case("draw", 255, 4, 8, 1, 1, 1, 4096, "random", "exact", 102),
    _case("draw", 256, 3, 11, (1 << 63) + 5, 1 << 40, 255, 1 << 40, BALANCED, "exact", 103),
    _case("draw", 257, 4, 8, M64, 1, 1 << 33, 0, SKEW4, "zero", 104),
    _case("draw", 4099, 3, 1, -7, 0, 1, 4096, "random", "exact", 105),
    _case("draw", 1 << 16, 2, 8, 1, 1, 255, 0, SKEW2, "exact", 106),
    _case("heads", 1, 1, 8, 1, 0, 0, 0, "random", "zero", 201),
    _case("heads", 255, 3, 512, M64, 1 << 40, 1 << 33, 1 << 40, BALANCED, "exact", 202),
    _case("heads", 256, 5, 8, (1 << 63) + 5, 1, 1, 0, "random", "zero", 203),
    _case("heads", 257, 7, 512, -7, 0, 255, 4096, "random", "exact", 204),
    _case("heads", 4099, 8, 8, 0, 1, 0, 4096, DECADES8, "exact", 205),
    _case("heads", 1 << 16, 3, 8, 1, 1 << 40, 255, 0, SKEW3, "zero", 206),
]
FUSED = _case("fused", 300, 3, 8, (1 << 63) + 5, 1, 255, 4096, "random", "exact", 301)
# the data-parallel property: a shard at env_offset draws rows env_offset.. of the draw over the global index
SHARD = _case("shard", 257, 3, 8, 1, 1, 1, 4096, "random", "zero", 401)


def quantise(x):
    return np.clip(np.round(np.asarray(x, dtype=np.float64) * 1024.0) / 1024.0, -8.0, 8.0)


def dist_logits(p):
    """Shared logits of the probabilities p, centred and rounded to the grid (so the law is the grid's, not p's)."""
    lp = np.log(np.asarray(p, dtype=np.float64))
    return quantise(lp - 0.5 * (lp.max() + lp.min()))


def case_inputs(case, rows=None):
    """(logits f64[rows, A], actor bias f64[A], v f32[rows], critic bias f32) of a case; rows defaults to n."""
    rows = case["n"] if rows is None else rows
    rs = np.random.RandomState(case["lseed"])
    A = case["A"]
    if case["dist"] == "random":
        logits = quantise(2.0 * rs.standard_normal((rows, A)))
    else:
        logits = np.broadcast_to(dist_logits(case["dist"]), (rows, A)).copy()
    ba = quantise(rs.uniform(-2.0, 2.0, A)) if case["bias"] == "exact" else np.zeros(A)
    v = rs.standard_normal(rows).astype(np.float32)  # any fp32: the value is one fp32 addition on both sides
    bc = np.float32(rs.standard_normal()) if case["bias"] == "exact" else np.float32(0.0)
    return logits, ba, v, bc


def case_expected(case):
    """(logp f64[n, A], action [n], gap [n], value f32[n]) on the host."""
    logits, _, v, bc = case_inputs(case)
    env = case["env_offset"] + np.arange(case["n"], dtype=np.uint64)
    logp, action, gap = expected_draw(logits, case["seed"], case["epoch"], case["step"], env)
    return logp, action, gap, v + bc
