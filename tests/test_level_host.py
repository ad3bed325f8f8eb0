"""CPU: level mode's host side against tests/level_ref.py -- the library's restatements of the draw
(merlin_level_draw_host) and of the scores (merlin_level_scores_host), merlin.levels.LevelSampler against hand-worked
cases, LevelSet.from_arrays' validation, and the new entries' argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import level_ref as R
from hand_map import HAND_GOAL, HAND_WALLS


def _cdfs():
    """name -> CDF: uniform ones, zero-weight levels at index 0, in the middle and last, one-hot ones."""
    out = {}
    for L in (1, 5, 5000):
        out[f"uniform{L}"] = np.arange(1, L + 1, dtype=np.float64) / L
    out["zero_first"] = R.cdf_of([0.0, 0.25, 0.25, 0.25, 0.25])
    out["zero_middle"] = R.cdf_of([0.3, 0.2, 0.0, 0.1, 0.4])
    out["zero_last"] = R.cdf_of([0.1, 0.2, 0.3, 0.4, 0.0])
    out["zeros"] = R.cdf_of([0.0, 0.5, 0.0, 0.5, 0.0])
    for hot in (0, 2, 4):
        out[f"one_hot{hot}"] = R.cdf_of(np.eye(5)[hot])
    w = np.random.RandomState(1).rand(5000)
    w[::7] = 0.0
    out["random5000"] = R.cdf_of(w / w.sum())
    return out


CDFS = _cdfs()


@pytest.mark.parametrize("name", sorted(CDFS))
@pytest.mark.parametrize("env_first", [0, (1 << 32) - 3, (1 << 40) + 5])
def test_draw_host_equals_restatement(name, env_first):
    from merlin import _native as nat

    cdf = CDFS[name]
    n, k_first, k_count = 70, 3, 33
    got = nat.level_draw_host(0x1234ABCD5, env_first, n, k_first, k_count, cdf)
    ref = R.draws(0x1234ABCD5, env_first, n, k_first, k_count, cdf)
    assert got.shape == (n, k_count) and (got == ref).all()
    assert got.min() >= 0 and got.max() < cdf.size
    w = np.diff(np.concatenate([[0.0], cdf]))
    assert not np.isin(got, np.flatnonzero(w == 0.0)).any()  # a zero-weight level is never drawn
    if cdf.size == 5 and (w > 0).sum() > 1:
        assert set(np.unique(got)) == set(np.flatnonzero(w > 0))  # 2310 draws: every weighted level turns up


def test_draw_host_key():
    """The draw depends on (seed, global env, k) only: a window of envs and draws is the same slice of a larger one,
    and another seed gives other levels."""
    from merlin import _native as nat

    cdf = CDFS["uniform5"]
    big = nat.level_draw_host(9, 100, 40, 0, 20, cdf)
    assert (nat.level_draw_host(9, 110, 7, 5, 6, cdf) == big[10:17, 5:11]).all()
    assert (nat.level_draw_host(10, 100, 40, 0, 20, cdf) != big).any()
    # a CDF of garbage keeps the index inside the bank
    bad = np.array([np.nan, -1.0, np.nan, 0.2, np.nan])
    got = nat.level_draw_host(9, 0, 50, 0, 10, bad)
    assert got.min() >= 0 and got.max() <= 4


SPECIAL = R.SPECIAL


@pytest.mark.parametrize("T,N,L", [(7, 130, 5), (3, 70, 5000), (2, 9, 1)])
@pytest.mark.parametrize("kind", [0, 1])
def test_scores_host_equals_restatement(T, N, L, kind):
    from merlin import _native as nat

    adv, lv = R.score_case(T, N, L, 3)
    s, c = nat.level_scores_host(adv, lv, L, kind)
    rs, rc = R.scores(adv, lv, L, kind)
    assert (s == rs).all() and (c == rc).all()
    # accumulate adds to what is there
    s2, c2 = nat.level_scores_host(adv[::-1].copy(), lv[::-1].copy(), L, kind, sum=s.copy(), count=c.copy(),
                                   accumulate=True)
    assert (s2 == 2 * rs).all() and (c2 == 2 * rc).all()


def test_step_scores_by_hand():
    """a = +-0 -> 0; NaN clamps (fminf keeps the number); inf and 40000 clamp to 32768 * 2^24 = 2^39; kind 1 drops
    the negative side; below 2^-25 rounds to 0, the tie 2^-25 to even (0), 3 * 2^-25 to 2."""
    from merlin import _native as nat

    lv = np.zeros((1, 1), dtype=np.int32)
    want0 = [0, 0, 1 << 39, 1 << 39, 1 << 39, 1 << 39, 1 << 39, 1 << 39, 0, 0, 0, 2, 1 << 23, 1 << 23, (1 << 24) + 2]
    want1 = [0, 0, 0, 1 << 39, 0, 1 << 39, 0, 1 << 39, 0, 0, 0, 2, 1 << 23, 0, (1 << 24) + 2]
    for kind, want in ((0, want0), (1, want1)):
        for a, w in zip(SPECIAL, want):
            s, c = nat.level_scores_host(np.array([[a]], dtype=np.float32), lv, 1, kind)
            assert int(s[0]) == w and int(c[0]) == 1, (kind, a)
            assert int(R.step_scores(a, kind)) == w, (kind, a)


def test_argument_checks():
    from merlin import _native as nat

    L = nat.lib()
    for s in ("merlin_env_set_levels", "merlin_env_set_level_cdf", "merlin_env_levels", "merlin_env_set_level_log",
              "merlin_level_draw_host",
              "merlin_level_scores", "merlin_level_scores_host"):
        assert s in nat.EXPORTED_SYMBOLS and getattr(L, s).argtypes is not None
    assert L.merlin_version() == nat.ABI_VERSION == 3
    vp = C.c_void_p
    cdf = np.ones(4)
    out = np.full((2, 2), 77, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    assert L.merlin_level_draw_host(1, 0, 2, 0, 2, p(cdf), 0, p(out)) == nat.E_INVALID
    assert L.merlin_level_draw_host(1, 0, 2, 0, 2, p(cdf), (1 << 20) + 1, p(out)) == nat.E_INVALID
    assert L.merlin_level_draw_host(1, 0, -1, 0, 2, p(cdf), 4, p(out)) == nat.E_INVALID
    assert L.merlin_level_draw_host(1, 0, 2, 0, 2, None, 4, p(out)) == nat.E_INVALID
    assert L.merlin_level_draw_host(1, 0, 0, 0, 2, None, 4, None) == nat.MERLIN_OK
    assert (out == 77).all()
    adv = np.zeros((2, 2), dtype=np.float32)
    lv = np.zeros((2, 2), dtype=np.int32)
    s = np.full(4, 5, dtype=np.int64)
    c = np.full(4, 5, dtype=np.int64)
    host = L.merlin_level_scores_host
    assert host(p(adv), p(lv), 2, 2, 4, 2, p(s), p(c), 0) == nat.E_INVALID  # kind
    assert host(p(adv), p(lv), 2, 2, 0, 0, p(s), p(c), 0) == nat.E_INVALID  # L
    assert host(p(adv), p(lv), 4097, 4096, 4, 0, p(s), p(c), 0) == nat.E_INVALID  # T N > 2^24
    assert host(p(adv), p(lv), -1, 2, 4, 0, p(s), p(c), 0) == nat.E_INVALID
    assert host(None, p(lv), 2, 2, 4, 0, p(s), p(c), 0) == nat.E_INVALID
    assert host(p(adv), p(lv), 2, 2, 4, 0, None, p(c), 0) == nat.E_INVALID
    assert (s == 5).all() and (c == 5).all()
    assert host(None, None, 0, 2, 4, 0, p(s), p(c), 0) == nat.MERLIN_OK  # no step: zeroed
    assert (s == 0).all() and (c == 0).all()
    # the device entries check their arguments before any device call
    assert L.merlin_level_scores(None, None, 2, 2, 4, 0, None, None, 0, None) == nat.E_INVALID
    assert L.merlin_env_set_levels(None, None, None, None, 0, 0, 0, None) == nat.E_INVALID
    assert L.merlin_env_set_level_cdf(None, None, None) == nat.E_INVALID
    assert L.merlin_env_levels(None, None, None, None) == nat.E_INVALID
    assert L.merlin_env_set_level_log(None, None) == nat.E_INVALID


# ------------------------------------------------------------------------------------------------------ the sampler
def _sampler(L, **kw):
    from merlin.levels import LevelSampler

    return LevelSampler(L, device="cpu", **kw)


def _feed(sm, scores, counts, iteration):
    """Levels with counts[l] > 0 get mean score scores[l] (exact in the fixed point: multiples of 2^-24)."""
    c = torch.tensor(counts, dtype=torch.int64)
    s = torch.tensor([int(round(x * R.SCALE)) * n for x, n in zip(scores, counts)], dtype=torch.int64)
    sm.update(s, c, iteration)


def _check_cdf(c):
    c = c.numpy()
    assert c.dtype == np.float64 and (np.diff(c) >= 0).all() and c[0] >= 0 and c[-1] == 1.0


def test_sampler_all_unseen_and_uniform():
    for strategy in ("uniform", "plr"):
        sm = _sampler(5, strategy=strategy)
        assert sm.weights().tolist() == [0.2] * 5
        assert sm.cdf().tolist() == [0.2, 0.4, 0.6000000000000001, 0.8, 1.0] or strategy == "uniform"
        _check_cdf(sm.cdf())
    sm = _sampler(4, strategy="uniform")
    _feed(sm, [1.0, 2.0, 3.0, 4.0], [1, 1, 1, 1], 1)  # scores are recorded and ignored
    assert sm.cdf().tolist() == [0.25, 0.5, 0.75, 1.0]


def test_sampler_all_seen_by_hand():
    """4 levels seen at iteration 1, scores 0.5, 2, 1, 0.25: ranks 3, 1, 2, 4.  beta = 1: P_S = (1/3, 1, 1/2, 1/4) /
    (25/12) = (4, 12, 6, 3) / 25.  Staleness is 0 everywhere: P_C is dropped, P = P_S."""
    sm = _sampler(4, strategy="plr", beta=1.0, rho=0.3)
    _feed(sm, [0.5, 2.0, 1.0, 0.25], [3, 1, 2, 7], 1)
    assert sm.score.tolist() == [0.5, 2.0, 1.0, 0.25]
    w = sm.weights().numpy()
    assert np.allclose(w, np.array([4, 12, 6, 3]) / 25.0, rtol=0, atol=1e-15)
    _check_cdf(sm.cdf())


def test_sampler_one_stale_by_hand():
    """As above, then iteration 3 sees levels 0, 1, 2 with the same scores: level 3 alone is stale (3 - 1 = 2), so
    P_C = (0, 0, 0, 1) and P = 0.7 P_S + 0.3 P_C = (2.8, 8.4, 4.2, 2.1 + 7.5) / 25."""
    sm = _sampler(4, strategy="plr", beta=1.0, rho=0.3)
    _feed(sm, [0.5, 2.0, 1.0, 0.25], [3, 1, 2, 7], 1)
    _feed(sm, [0.5, 2.0, 1.0, 0.0], [1, 1, 1, 0], 3)
    assert sm.last_seen.tolist() == [3, 3, 3, 1] and sm.score.tolist() == [0.5, 2.0, 1.0, 0.25]
    w = sm.weights().numpy()
    assert np.allclose(w, np.array([2.8, 8.4, 4.2, 9.6]) / 25.0, rtol=0, atol=1e-15)
    _check_cdf(sm.cdf())


def test_sampler_ties_and_unseen_by_hand():
    """6 levels, 1 and 4 unseen (1/6 each); the seen ones share 4/6.  Scores (1, -, 2, 1, -, 1): level 2 is rank 1, the
    three-way tie goes by index -- levels 0, 3, 5 are ranks 2, 3, 4.  beta = 0.5: P_S ~ rank^-2 = (1/4, 1, 1/9, 1/16),
    sum 205/144 -> (36, 144, 16, 9) / 205.  Seen at iteration 2 except level 5 (iteration 1): P_C = (0, 0, 0, 1)."""
    sm = _sampler(6, strategy="plr", beta=0.5, rho=0.2)
    _feed(sm, [0, 0, 0, 0, 0, 1.0], [0, 0, 0, 0, 0, 4], 1)
    _feed(sm, [1.0, 0, 2.0, 1.0, 0, 0], [2, 0, 5, 1, 0, 0], 2)
    assert sm.seen.tolist() == [True, False, True, True, False, True]
    ps = np.array([36, 144, 16, 9]) / 205.0
    pseen = 0.8 * ps + 0.2 * np.array([0, 0, 0, 1.0])
    want = np.full(6, 1 / 6)
    want[[0, 2, 3, 5]] = pseen * (4 / 6)
    assert np.allclose(sm.weights().numpy(), want, rtol=0, atol=1e-15)
    _check_cdf(sm.cdf())
    assert abs(float(sm.weights().sum()) - 1.0) < 1e-15


def test_sampler_large_beta_is_uniform_over_seen():
    sm = _sampler(5, strategy="plr", beta=1e12, rho=0.0)
    _feed(sm, [3.0, 1.0, 0, 2.0, 0], [1, 1, 0, 1, 0], 1)
    assert np.allclose(sm.weights().numpy(), 0.2, rtol=0, atol=1e-10)


@pytest.mark.parametrize("L", [4, 6, 257])
def test_sampler_equals_restatement_over_updates(L):
    """Random updates (levels dropping in and out, tied scores): weights and CDF against level_ref.Sampler.  On the
    CPU torch and numpy run the same float64 operations in the same order except pow and the sums' association:
    1e-14 absolute on values <= 1 leaves them a few hundred ulps."""
    rs = np.random.RandomState(L)
    sm, ref = _sampler(L, strategy="plr", beta=0.3, rho=0.25), R.Sampler(L, "plr", 0.3, 0.25)
    for it in range(1, 6):
        c = rs.randint(0, 3, size=L) * rs.randint(1, 50, size=L)
        s = c * rs.randint(0, 4, size=L) * (1 << 22)  # means from {0, 0.25, 0.5, 0.75}: many ties
        sm.update(torch.from_numpy(s), torch.from_numpy(c), it)
        ref.update(s, c, it)
        assert (sm.score.numpy() == ref.score).all() and (sm.seen.numpy() == ref.seen).all()
        assert (sm.last_seen.numpy() == ref.last_seen).all()
        assert np.abs(sm.weights().numpy() - ref.weights()).max() <= 1e-14
        assert np.abs(sm.cdf().numpy() - ref.cdf()).max() <= 1e-14
        _check_cdf(sm.cdf())


def test_sampler_rejects_bad_arguments():
    from merlin.levels import LevelSampler

    for kw in (dict(strategy="greedy"), dict(score="td"), dict(beta=0.0), dict(rho=1.5)):
        with pytest.raises(ValueError):
            LevelSampler(4, device="cpu", **kw)
    with pytest.raises(ValueError):
        LevelSampler(0, device="cpu")


# ------------------------------------------------------------------------------------------------------- LevelSet
def _hand(**over):
    d = dict(walls=[list(HAND_WALLS)], goal=[list(HAND_GOAL)], agent=[[1, 1, 0, 0]])
    d.update(over)
    return d


def test_from_arrays_accepts_the_hand_map_and_round_trips(tmp_path):
    from merlin.levels import LevelSet

    ls = LevelSet.from_arrays(**_hand(), solvable=True)
    assert len(ls) == 1 and ls.size == 5 and ls.device.type == "cpu"
    assert ls.walls.dtype == ls.goal.dtype == ls.agent.dtype == torch.int32
    assert ls.walls.tolist() == [list(HAND_WALLS)] and ls.agent.tolist() == [[1, 1, 0, 0]]
    two = LevelSet.from_arrays(walls=[HAND_WALLS, HAND_WALLS], goal=[HAND_GOAL, (1, 1)], agent=[[1, 1, 3], [3, 1, 2]])
    two.seeds, two.difficulties = [7, 1 << 40], ["easy", "hard"]
    path = str(tmp_path / "set.npz")
    two.save(path)
    back = LevelSet.load(path)
    for f in ("walls", "goal", "agent"):
        assert torch.equal(getattr(back, f), getattr(two, f))
    assert back.size == 5 and back.seeds == [7, 1 << 40] and back.difficulties == ["easy", "hard"]
    # size 32: the top bit is a wall bit, not a sign
    S = 32
    rows = [0xFFFFFFFF] + [0x80000001] * (S - 2) + [0xFFFFFFFF]
    big = LevelSet.from_arrays([rows], [[30, 30]], [[1, 1, 1]], solvable=True)
    assert (big.walls.numpy().view(np.uint32) == np.array(rows, dtype=np.uint32)).all()


@pytest.mark.parametrize("over,what", [
    (dict(walls=[[31, 17, 31, 31, 30]]), "border"),  # a hole in the bottom row
    (dict(walls=[[31, 16, 31, 31, 31]]), "border"),  # a hole in the left column
    (dict(walls=[[31, 17 + 32, 31, 31, 31]]), "beyond"),  # a bit outside the grid
    (dict(agent=[[1, 2, 0, 0]]), "agent"),  # on a wall
    (dict(agent=[[5, 1, 0, 0]]), "agent"),  # outside the grid
    (dict(goal=[[2, 2]]), "goal"),  # on a wall
    (dict(goal=[[-1, 1]]), "goal"),
    (dict(goal=[[1, 1]]), "stands on the goal"),
    (dict(agent=[[1, 1, 4, 0]]), "direction"),
    (dict(agent=[[1, 1, -1, 0]]), "direction"),
    (dict(goal=[[3, 1], [3, 1]]), "goal is"),  # a count mismatch
    (dict(walls=[[15, 9, 9, 15]], goal=[[1, 1]], agent=[[2, 2, 0, 0]]), "size"),  # size 4
    (dict(walls=[[31.0, 17.0, 31.0, 31.0, 31.0]]), "integer"),
])
def test_from_arrays_rejects(over, what):
    from merlin.levels import LevelSet

    with pytest.raises(ValueError, match=what):
        LevelSet.from_arrays(**_hand(**over))


def test_from_arrays_solvable():
    """The goal walled off from the agent: accepted as a map, rejected when asked for solvable ones."""
    from merlin.levels import LevelSet

    walls = [127, 65, 65 + 8, 127, 65, 65, 127]  # 7x7: rows 1-2 and rows 4-5 are separate rooms
    LevelSet.from_arrays([walls], [[1, 4]], [[1, 1, 0]])
    with pytest.raises(ValueError, match="level 0: the goal cannot be reached"):
        LevelSet.from_arrays([walls], [[1, 4]], [[1, 1, 0]], solvable=True)
    LevelSet.from_arrays([walls], [[5, 2]], [[1, 1, 0]], solvable=True)
