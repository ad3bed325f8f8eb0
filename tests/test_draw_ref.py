"""CPU: the host restatement of the acting draw (tests/draw_ref.py) on its own -- the hash against published
splitmix64 outputs, the range of the uniforms, the law of the race against the softmax (chi-square over 2^20 decisions
per distribution), independence across envs, steps, epochs and seeds (contingency chi-square), the power of a
decision-by-decision comparison against single mistakes in the key or the score, and the margin condition on the fixed
case list that tests/test_gpu_draw.py runs on the device.  Every threshold is the upper 1e-6 quantile of the chi-square
law at the test's degrees of freedom; seeds are fixed, so nothing here is random."""
import numpy as np
import pytest

import draw_ref as D

N = 1 << 20


def test_mix64_known_answers():
    """The first three outputs of splitmix64 seeded with 0 (state += golden ratio, output = finaliser)."""
    g = D.K_SEED
    assert int(D.mix64(g)) == 0xe220a8397b1dcdaf
    assert int(D.mix64(2 * g)) == 0x6e789e6aa1b965f4
    assert int(D.mix64(3 * g)) == 0x06c45d188009454f
    assert D.mix64(np.array([g, 2 * g & D.M64], dtype=np.uint64)).tolist() == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4]


def test_hash_is_four_chained_finalisers_and_seeds_wrap():
    def by_hand(seed, epoch, step, env, j):  # Python integers, masked by hand
        x = int(D.mix64((seed + D.K_SEED) & D.M64))
        x = int(D.mix64(x ^ ((epoch + D.K_EPOCH) & D.M64)))
        x = int(D.mix64(x ^ ((step * D.K_STEP) & D.M64)))
        return int(D.mix64(x ^ ((env * D.K_ENV + j) & D.M64)))

    for key in [(0, 0, 0, 0, 0), (123, 3, 5, 77, 2), (D.M64, 1 << 40, 1 << 33, (1 << 40) + 4098, 7)]:
        assert int(D.hash64(*key)) == by_hand(*key)
        assert float(D.uniform01(*key)) == ((by_hand(*key) >> 11) + 1) / 2.0 ** 53
    # seeds modulo 2^64, as merlin._native masks them
    assert int(D.hash64(-7, 1, 2, 3, 1)) == int(D.hash64((1 << 64) - 7, 1, 2, 3, 1))
    assert int(D.hash64((1 << 64) + 9, 1, 2, 3, 1)) == int(D.hash64(9, 1, 2, 3, 1))
    # vectorised == scalar
    env = np.arange(5, dtype=np.uint64) + np.uint64(1 << 40)
    u = D.uniform01(9, 2, 255, env[:, None], np.arange(8)[None, :])
    assert u.shape == (5, 8) and float(u[3, 6]) == float(D.uniform01(9, 2, 255, (1 << 40) + 3, 6))


def test_uniform_range():
    assert float(D.bits_to_uniform(D.M64)) == 1.0                       # all ones: the only way to 1
    assert float(D.bits_to_uniform(D.M64 - (1 << 11))) == 1.0 - 2.0 ** -53
    assert float(D.bits_to_uniform(D.M64 ^ (1 << 63))) < 1.0
    assert float(D.bits_to_uniform(0)) == 2.0 ** -53 > 0.0              # never 0: log(-log u) stays finite or +inf
    assert float(D.bits_to_uniform((1 << 11) - 1)) == 2.0 ** -53        # the low 11 bits are dropped
    u = D.uniform01(5, 1, 2, np.arange(N, dtype=np.uint64)[:, None], np.arange(4)[None, :])
    assert u.min() > 0.0 and u.max() <= 1.0
    assert abs(u.mean() - 0.5) < 5 * (1 / 12 / u.size) ** 0.5


def test_chi2_quantiles():
    assert abs(D.chi2_upper(2) - 27.631) < 1e-3  # 2 ln 1e6
    for df, x in [(1, 3.841459), (3, 7.814728), (4, 9.487729), (7, 14.06714)]:  # the textbook 5 % points
        assert abs(D.chi2_upper(df, 0.05) - x) < 1e-4
    try:
        from scipy.stats import chi2
    except ImportError:
        return
    for df in (1, 2, 3, 4, 7, 8):
        assert abs(D.chi2_upper(df) - chi2.isf(1e-6, df)) < 1e-6 * chi2.isf(1e-6, df)


def _actions(logits, seed=11, epoch=3, n=N):
    """n decisions of one distribution, spread over 64 steps x n / 64 envs."""
    k = np.arange(n, dtype=np.uint64)
    step, env = k & np.uint64(63), k >> np.uint64(6)
    logp = D.log_softmax64(logits)
    u = D.uniform01(seed, epoch, step[:, None], env[:, None], np.arange(logp.shape[-1])[None, :])
    return D.race(np.broadcast_to(logp, u.shape), u)[0], np.exp(logp)


@pytest.mark.parametrize("p", [D.NEAR_UNIFORM, D.SKEW3, D.SKEW4, D.SKEW2, D.DECADES8, D.BALANCED],
                         ids=lambda p: "p%g-A%d" % (p[0], len(p)))
def test_law_matches_softmax(p):
    a, prob = _actions(D.dist_logits(p), seed=len(p) * 1000 + 17)
    counts = np.bincount(a, minlength=len(p)).astype(np.float64)
    chi2 = float(((counts - N * prob) ** 2 / (N * prob)).sum())
    bound = D.chi2_upper(len(p) - 1)
    print(f"law {p}: chi2 {chi2:.2f} < {bound:.2f}, counts {counts.astype(int).tolist()}")
    assert (N * prob).min() > 50  # the chi-square approximation holds in every cell
    assert chi2 < bound


def test_single_action_always_drawn():
    logp, a, gap = D.expected_draw(np.array([[3.25]]), 5, 1, 2, np.arange(N, dtype=np.uint64))
    assert (a == 0).all() and np.isinf(gap).all() and (logp == 0.0).all()


def _contingency(x, y, A):
    table = np.bincount(x * A + y, minlength=A * A).reshape(A, A).astype(np.float64)
    exp = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / table.sum()
    return float(((table - exp) ** 2 / exp).sum()), float(exp.min())


@pytest.mark.parametrize("p", [D.BALANCED, D.SKEW3], ids=["balanced", "skewed"])
@pytest.mark.parametrize("axis", ["env", "step", "epoch", "seed"])
def test_neighbouring_keys_draw_independently(axis, p):
    """Actions at (k, k + 1) along one key coordinate, N disjoint pairs, the other coordinates varied too."""
    logp = D.log_softmax64(D.dist_logits(p))
    A = len(p)
    k = np.arange(N, dtype=np.uint64)
    lo, hi, two = k & np.uint64(255), k >> np.uint64(8), np.uint64(2)
    const = lambda v: np.full(N, v, dtype=np.uint64)  # noqa: E731
    # the paired coordinate runs over the even values 2m and its neighbour is 2m + 1: N disjoint pairs
    key = {"env": dict(seed=const(77), epoch=const(5), step=lo, env=two * hi),
           "step": dict(seed=const(77), epoch=const(5), step=two * lo, env=hi),
           "epoch": dict(seed=const(77), epoch=two * lo, step=const(3), env=hi),
           "seed": dict(seed=two * hi, epoch=const(5), step=const(3), env=lo)}[axis]
    j = np.arange(A)[None, :]
    col = {n: v[:, None] for n, v in key.items()}
    x = D.race(logp, D.uniform01(col["seed"], col["epoch"], col["step"], col["env"], j))[0]
    col[axis] = col[axis] + np.uint64(1)
    y = D.race(logp, D.uniform01(col["seed"], col["epoch"], col["step"], col["env"], j))[0]
    chi2, least = _contingency(x, y, A)
    bound = D.chi2_upper((A - 1) ** 2)
    print(f"independence {axis} {p}: chi2 {chi2:.2f} < {bound:.2f} (least expected cell {least:.1f})")
    assert least > 20
    assert chi2 < bound


def test_single_mistakes_are_visible_decision_by_decision():
    """At a balanced distribution every single mistake in the key or the score turns at least 20 % of the decisions, so
    an equality check against expected_draw tells them apart; at the 0.97 case alone some would hide (both draws
    mostly land on the likely action), which is why every device case list holds a balanced case."""
    n, off = 1 << 16, 4096
    seed, epoch, step = 9, 3, 5
    env = off + np.arange(n, dtype=np.uint64)
    j = np.arange(3)[None, :]
    turned = {}
    for name, p in (("balanced", D.BALANCED), ("skewed", D.SKEW3)):
        logp = D.log_softmax64(D.dist_logits(p))
        good = D.expected_draw(D.dist_logits(p), seed, epoch, step, env)[1]
        u = D.uniform01(seed, epoch, step, env[:, None], j)
        wrong = {
            "env + 1": D.expected_draw(D.dist_logits(p), seed, epoch, step, env + np.uint64(1))[1],
            "step + 1": D.expected_draw(D.dist_logits(p), seed, epoch, step + 1, env)[1],
            "epoch + 1": D.expected_draw(D.dist_logits(p), seed, epoch + 1, step, env)[1],
            "j + 1": D.race(logp, D.uniform01(seed, epoch, step, env[:, None], j + 1))[0],
            "env_offset dropped": D.expected_draw(D.dist_logits(p), seed, epoch, step, env - np.uint64(off))[1],
            "u -> 1 - u": D.race(logp, 1.0 - u)[0],
        }
        turned[name] = {m: float((a != good).mean()) for m, a in wrong.items()}
        print(name, {m: round(v, 4) for m, v in turned[name].items()})
    assert len(turned["balanced"]) == 6 and min(turned["balanced"].values()) >= 0.20
    assert min(turned["skewed"].values()) < 0.20  # the skewed case alone could not


ALL_CASES = D.CASES + [D.FUSED, D.SHARD]


def test_case_list_covers_the_issue_lists():
    draw = [c for c in D.CASES if c["entry"] == "draw"]
    heads = [c for c in D.CASES if c["entry"] == "heads"]
    assert {c["A"] for c in draw} == {1, 2, 3, 4} and {c["A"] for c in heads} == {1, 3, 5, 7, 8}
    assert {c["width"] for c in draw} >= {1, 8} and max(c["width"] for c in draw) > 8
    assert {c["width"] for c in heads} == {8, 512}
    for entry in (draw, heads):
        assert {c["n"] for c in entry} == {1, 255, 256, 257, 4099, 1 << 16}
        assert any(c["dist"] == D.BALANCED for c in entry) and any(c["dist"] == "random" for c in entry)
        assert any(isinstance(c["dist"], tuple) and c["dist"][0] > 0.9 or c["dist"] == D.SKEW4 for c in entry)
    assert {c["seed"] for c in D.CASES} == {0, 1, (1 << 63) + 5, D.M64, -7}
    assert {c["epoch"] for c in D.CASES} == {0, 1, 1 << 40}
    assert {c["step"] for c in D.CASES} == {0, 1, 255, 1 << 33}
    assert {c["env_offset"] for c in D.CASES} == {0, 4096, 1 << 40}
    assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["id"] for c in ALL_CASES])
def test_case_inputs_are_exact_and_clear_of_the_margin(case):
    logits, ba, v, bc = D.case_inputs(case)
    assert logits.shape == (case["n"], case["A"]) and v.dtype == np.float32
    # exact in fp32, with the shift through act_heads' ReLU and with the biases
    for x in (logits, ba, logits - ba, logits + D.SHIFT - ba):
        assert (x.astype(np.float32).astype(np.float64) == x).all() and (x * 1024 == np.round(x * 1024)).all()
    assert (logits + D.SHIFT - ba > 0).all()
    assert (logits.max(-1) - logits.min(-1) <= 16).all()
    _, action, gap, _ = D.case_expected(case)
    under = int((gap <= case["margin"]).sum())  # what the device comparison excuses
    print(f"{case['id']}: {case['n']} decisions, {under} under the margin {case['margin']:g}")
    assert case["margin"] == D.MARGIN
    assert under <= D.EXCUSED_CAP * case["n"]
    if case["n"] < D.EXACT_BELOW:
        assert under == 0
    if case["A"] > 1 and case["n"] >= 255:
        assert len(np.unique(action)) > 1
