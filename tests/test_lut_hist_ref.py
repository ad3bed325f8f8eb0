"""CPU: tests/lut_hist_ref.py (the conv2 table histogram restated) against exact rational and integer
arithmetic, so that tests/test_gpu_conv2lut_seams.py can hold the kernels to it bit for bit."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import lut_hist_ref as R
from test_conv2_tables import lut2_rows


def _f32(x):
    return float(np.float32(x))


def _round_half_away(g: float, K: int) -> int:
    x = abs(Fraction(g)) * Fraction(2) ** K + Fraction(1, 2)
    q = x.numerator // x.denominator
    return -q if g < 0 else q


def _check_to_fixed(vals, K):
    vals = [_f32(v) for v in vals]
    got = R.to_fixed(torch.tensor(vals, dtype=torch.float32), K).tolist()
    for v, q in zip(vals, got):
        assert q == _round_half_away(v, K), (v.hex(), K, q)


def test_to_fixed_crafted_values():
    K = 10
    u = 2.0 ** -K
    up, dn = (lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))), \
             (lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf))))
    ties = [0.5 * u, 1.5 * u, 2.5 * u, 1023.5 * u, 4097.5 * u]
    vals = [0.0, -0.0]
    for t in ties:  # exact ties of both signs and both float32 neighbours of each
        vals += [t, -t, up(t), dn(t), -up(t), -dn(t)]
    vals += [2.0 ** k for k in range(-30, 12)] + [-(2.0 ** k) for k in range(-30, 12)]
    vals += [dn(2.0 ** 12), -dn(2.0 ** 12), 0.25 * u, dn(0.5 * u) / 2, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -127]
    _check_to_fixed(vals, K)
    # ties are resolved away from zero, not to even
    assert R.to_fixed(torch.tensor([0.5 * u, -0.5 * u, 1.5 * u, -1.5 * u, 2.5 * u], dtype=torch.float32), K).tolist() \
        == [1, -1, 2, -2, 3]


def test_to_fixed_denormals_and_values_just_under_the_bound():
    # K as the kernel would choose it for a subnormal / a tiny normal / a huge bound at n = 1 (lg = 5)
    for M in (2.0 ** -140, 1.5 * 2.0 ** -126, 2.0 ** -120, 3.0, 2.0 ** 100):
        K = R.fixed_exp(M, 1)
        dn = float(np.nextafter(np.float32(M), np.float32(0)))
        sub = [m * 2.0 ** -149 for m in (1, 2, 3, 0x7fffff, 0x400001) if m * 2.0 ** -149 <= M]
        _check_to_fixed([M, -M, dn, -dn, M / 2, M / 3, M * 2.0 ** -30] + sub + [-s for s in sub], K)
        assert abs(R.to_fixed(torch.tensor([M], dtype=torch.float32), K).item()) < 2 ** (62 - 5)


@pytest.mark.parametrize("scale", [-140, -126, -100, -20, 0, 13, 100])
def test_to_fixed_random_floats(scale):
    rs = np.random.RandomState(1000 + scale)
    # 24 random significant bits over 45 binades below 2^scale (subnormals included at the two lowest scales)
    v = (rs.randint(1 << 23, 1 << 24, size=3000).astype(np.float64) * 2.0 ** -24
         * 2.0 ** (scale - rs.randint(0, 45, size=3000)) * rs.choice([-1.0, 1.0], size=3000)).astype(np.float32)
    M = float(np.abs(v).max())
    for n, loose in ((1, 1.0), (300, 1.0), (41943, 1024.0)):
        _check_to_fixed(v.tolist(), R.fixed_exp(_f32(M * loose), n))


def test_fixed_exp_inequalities():
    ns = [1, 2, 3, 5, 40, 41, 163, 164, 1310, 1311, 2621, 2622, 41943, 41944, 199999]
    Ms = [0.0, 2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -126, 0.75, 1.0, float(np.nextafter(np.float32(1), np.float32(0))),
          4.0, 5.3, 2.0 ** 100, float(np.finfo(np.float32).max)]
    for n in ns:
        for M in Ms:
            M = _f32(M)
            K = R.fixed_exp(M, n)
            e = math.frexp(M)[1]
            lg = 62 - e - K
            assert Fraction(M) < Fraction(2) ** e                       # the bound is strict
            assert M == 0.0 or Fraction(M) >= Fraction(2) ** (e - 1)    # and e is the smallest such
            assert 2 ** lg >= 25 * n + 1 > 2 ** (lg - 1)
            assert 25 * n * 2 ** (62 - lg) < 2 ** 62                    # 25 n terms below 2^(62 - lg) each
    # the one n below 200,000 with 25 n + 1 a power of two: the comparison is decided by equality
    assert [n for n in range(1, 200000) if (25 * n + 1) & (25 * n) == 0] == [41943]
    assert R.fixed_exp(0.75, 41943) == 62 - 20 and R.fixed_exp(0.75, 41944) == 62 - 21
    assert R.fixed_exp(0.75, 1310) == 62 - 15 and R.fixed_exp(0.75, 1311) == 62 - 16
    assert R.fixed_exp(4.0, 1) == 62 - 5 - 3 and R.fixed_exp(0.0, 1) == 62 - 5


@pytest.mark.parametrize("n,T,scale,loose", [(1, 2, 0, 1.0), (3, 1, -100, 1.0), (6, 2, 0, 1024.0), (4, 2, 100, 1.0),
                                            (4, 1, -130, 8.0)])
def test_hist_and_fold_match_integer_arithmetic(n, T, scale, loose):
    rs = np.random.RandomState(n)
    c = rs.randint(0, 5, size=(n, 49))
    rows = lut2_rows(c).reshape(n * 25, 16)
    g = (rs.randn(T, n * 25, 64) * 2.0 ** (scale - rs.randint(0, 40, size=(T, n * 25, 64)))).astype(np.float32)
    g[rs.rand(*g.shape) < 0.3] = 0.0
    M = _f32(float(np.abs(g).max()) * loose)
    K = R.fixed_exp(M, n)
    acc = R.hist(torch.from_numpy(rows), torch.from_numpy(g), M, n)
    dT = R.fold(acc, K)
    ref64, count = R.hist64(torch.from_numpy(rows), torch.from_numpy(g))
    want = np.zeros((T, R.NROW, 64), dtype=object)
    cnt = np.zeros((T, R.NROW, 64), dtype=np.int64)
    exact = np.zeros((T, R.NROW, 64), dtype=object)
    for t in range(T):
        for i in range(n * 25):
            q = np.array([_round_half_away(float(v), K) for v in g[t, i]], dtype=object)
            fr = np.array([int(Fraction(float(v)) * 2 ** 149) for v in g[t, i]], dtype=object)  # units of 2^-149
            for k in range(16):
                want[t, rows[i, k]] += q
                exact[t, rows[i, k]] += fr
                cnt[t, rows[i, k]] += g[t, i] != 0
    assert (acc.numpy().astype(object) == want).all()
    assert (count.numpy() == cnt).all()
    got, r64, touched = dT.numpy().ravel(), ref64.numpy().ravel(), np.flatnonzero(cnt.ravel())
    assert not got[cnt.ravel() == 0].any() and not r64[cnt.ravel() == 0].any()
    # the float64 reference and the bound the GPU tests use: the exact sums sit inside it
    tol = R.tolerance(ref64, count, K).numpy().ravel()
    gmax = Fraction(float(np.abs(g).max()))
    for j in touched:
        folded = np.float32(math.ldexp(float(int(want.ravel()[j])), -K))
        assert got[j] == folded
        ex = Fraction(int(exact.ravel()[j]), 2 ** 149)
        # float64 adds of cnt terms below gmax: each partial sum is below cnt * gmax and rounds by 2^-53 of itself
        assert abs(Fraction(float(r64[j])) - ex) <= int(cnt.ravel()[j]) ** 2 * gmax * Fraction(2) ** -53
        assert abs(Fraction(float(folded)) - ex) <= Fraction(float(tol[j])) * (1 + Fraction(2) ** -20)


def test_tap_row_ranges_partition_the_table():
    seen = sorted(r for k in range(16) for r in R.tap_row_range(k))
    assert seen == list(range(R.NROW))
    rs = np.random.RandomState(0)
    rows = lut2_rows(rs.randint(0, 5, size=(500, 49))).reshape(-1, 16)
    for k in range(16):
        rr = R.tap_row_range(k)
        assert set(np.unique(rows[:, k])) <= set(rr)
    assert list(R.tap_row_range(0)) == [0, 4, 8, 12, 16]
