"""CPU: the library's host restatements of the sampled-policy passes (merlin_policy_chain_host: a recursion over a
successor table with an absorbing goal state; merlin_policy_occupancy_host: a scatter over the same table) against the
tests' own numpy restatement (tests/policy_chain_ref.py: whole-array shifts), on the CPU oracle's maps at every grid
size of test_gpu_env_sizes' matrix up to 17 and on one map at 31 and 32; the forward / backward identities; the exact
agreement with merlin_policy_paths_host under one-hot probabilities; a closed form that pins truncation at T; and
merlin.sampled_field's torch side on a 5x5 map small enough to work out by hand.

Tolerances (derived, not measured): float64 sums of at most T <= 4,096 steps with under 10 roundings of 2^-53 each stay
below 5e-12 relative on quantities bounded by 1 (success, ret, disc, hit) or by T (steps, visits): 1e-9 and 1e-9 T."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pathing_ref import P_FWD
from policy_chain_ref import chain_ref, corridor_closed_form, dirichlet_field, occupancy_ref, one_hot, reward
from policy_field_ref import CASES, bouncer_field
from test_policy_field_host import HAND_DIST, HAND_GOAL, HAND_WALLS, M9, _maps, random_field

TOL = 1e-9
SMALL = [(d, s) for d, s in CASES if s <= 17]
BIG = [("mediumhard", 31), ("hardest", 32)]
HOST_CASES = [(d, s, M9) for d, s in SMALL] + [(d, s, 1) for d, s in BIG]
HOST_IDS = [f"{d}-{s}-m{m}" for d, s, m in HOST_CASES]
CHAIN = ("success", "ret", "steps", "disc")


def horizons(size):
    return (1, 2, 37, 4 * size * size)


def clean_random_field(size, seed, m):
    """random_field with its few actions outside {0, 1, 2} turned into left turns: a one-hot row needs an action."""
    a = random_field(size, seed, m)
    return np.where((a < 0) | (a > 2), 0, a).astype(np.int8)


@functools.lru_cache(maxsize=None)
def prob_fields(diff, size, m):
    """name -> (probs float32[m, 4, S, S, 3], the action field behind a one-hot one or None); shared, never written."""
    cells = _maps(diff, size)[0][:m]
    rnd = clean_random_field(size, 13 * size + len(diff), m)
    bnc = np.stack([bouncer_field(c) for c in cells])
    out = {"dirichlet": (dirichlet_field(m, size, 5 * size + len(diff)), None),
           "p_fwd": (np.broadcast_to(np.array(P_FWD, dtype=np.float32), (m, 4, size, size, 3)).copy(), None),
           "onehot_random": (one_hot(rnd), rnd), "onehot_bouncer": (one_hot(bnc), bnc)}
    for p, _ in out.values():
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(diff, size, m, name, T, gamma=0.99):
    """(chain_ref's dict, visits, hit) of one case, computed once and shared (the GPU tests use it too)."""
    cells, _, goal, start = (a[:m] for a in _maps(diff, size))
    probs = prob_fields(diff, size, m)[name][0]
    ch = chain_ref(cells, goal, probs, T, gamma)
    vis, hit = occupancy_ref(cells, goal, probs, start, T)
    for a in list(ch.values()) + [vis, hit]:
        a.setflags(write=False)
    return ch, vis, hit


def close(got, want, tol, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert (np.isnan(got) == np.isnan(want)).all(), what
    err = np.nanmax(np.abs(got - want)) if np.isfinite(want).any() else 0.0
    assert err <= tol, (what, err, tol)


def check_identities(ch, vis, hit, start, T, what):
    """sum_t hit = success[start], sum_t hit r_t = ret[start], sum_p visits = steps[start], per map."""
    i = (np.arange(len(start)), start[:, 2], start[:, 1], start[:, 0])
    r = np.array([reward(t, T) for t in range(1, T + 1)])
    assert np.abs(hit.sum(1) - ch["success"][i]).max() <= TOL, what
    assert np.abs((hit * r).sum(1) - ch["ret"][i]).max() <= TOL, what
    assert np.abs(vis.sum((1, 2, 3)) - ch["steps"][i]).max() <= TOL * T, what


@pytest.mark.parametrize("diff,size,m", HOST_CASES, ids=HOST_IDS)
def test_host_equals_numpy(diff, size, m):
    from merlin import _native as nat

    cells, walls, goal, start = (a[:m] for a in _maps(diff, size))
    start = start.copy()
    start[:, 3] = 0
    wall = np.broadcast_to((cells == 1)[:, None], (m, 4, size, size))
    for name, (probs, _) in prob_fields(diff, size, m).items():
        for T in horizons(size):
            want, wvis, whit = reference(diff, size, m, name, T)
            got = dict(zip(CHAIN, nat.policy_chain_host(walls, goal, probs, size, T, gamma=0.99)))
            for k in CHAIN:
                close(got[k], want[k], TOL * T if k == "steps" else TOL, (name, T, k))
                assert np.isnan(got[k][wall]).all() and np.isfinite(got[k][~wall]).all()
            assert (got["success"][~wall] >= 0).all() and (got["success"][~wall] <= 1 + TOL).all()
            vis, hit = nat.policy_occupancy_host(walls, goal, probs, start, size, T)
            close(vis, wvis, TOL * T, (name, T, "visits"))
            close(hit, whit, TOL, (name, T, "hit"))
            assert (vis[wall] == 0).all() and hit.shape == (m, T)
            check_identities(got, vis, hit, start, T, (name, T))
            check_identities(want, wvis, whit, start, T, (name, T, "ref"))
    # the requested outputs alone, the others null: the same values
    probs = prob_fields(diff, size, m)["dirichlet"][0]
    full = nat.policy_chain_host(walls, goal, probs, size, 37)
    for j, k in enumerate(CHAIN):
        alone = nat.policy_chain_host(walls, goal, probs, size, 37, outputs=(k,))
        assert [a is not None for a in alone] == [i == j for i in range(4)]
        assert np.array_equal(alone[j], full[j], equal_nan=True)
    v, h = nat.policy_occupancy_host(walls, goal, probs, start, size, 37)
    assert np.array_equal(nat.policy_occupancy_host(walls, goal, probs, start, size, 37, outputs=("visits",))[0], v)
    assert np.array_equal(nat.policy_occupancy_host(walls, goal, probs, start, size, 37, outputs=("hit",))[1], h)


def one_hot_identity(paths, chain, T):
    """With one-hot probabilities the chain is the functional graph merlin_policy_paths searches: exact."""
    success, ret, steps, _ = chain
    free = paths != -1
    inside = (paths >= 1) & (paths <= T)
    live = ~np.isnan(success)
    assert (live | ~free).all()
    assert (success[live] == inside[live].astype(np.float64)).all()
    assert (steps[live] == np.where(inside, paths, T)[live].astype(np.float64)).all()
    want = np.where(inside, 1.0 - 0.9 * (paths.astype(np.float64) / float(T)), 0.0)
    assert (ret[live] == want[live]).all()


@pytest.mark.parametrize("diff,size,m", HOST_CASES, ids=HOST_IDS)
def test_one_hot_equals_policy_paths(diff, size, m):
    from merlin import _native as nat

    _, walls, goal, _ = (a[:m] for a in _maps(diff, size))
    seen = 0
    for name in ("onehot_random", "onehot_bouncer"):
        probs, action = prob_fields(diff, size, m)[name]
        paths = nat.policy_paths_host(walls, goal, action, size)
        for T in horizons(size):
            one_hot_identity(paths, nat.policy_chain_host(walls, goal, probs, size, T), T)
        seen += int((paths >= 1).sum())
    assert seen > 0 or (diff, size) == ("easy", 5)  # some pose does arrive (easy 5: no cell faces the goal)


def hand_map(q, copies=1):
    """test_policy_field_host's corridor (1, 1) (2, 1) (3, 1) with the goal on its last cell.  On (2, 1) the pose
    facing the goal (dir 0) goes forward with probability q and turns left with 1 - q; every other pose of the map
    turns left with probability 1, so the poses of (1, 1) and (3, 1) never leave their cell."""
    S = 5
    walls = np.array([HAND_WALLS] * copies, dtype=np.uint32)
    goal = np.array([HAND_GOAL] * copies, dtype=np.int32)
    probs = np.zeros((copies, 4, S, S, 3), dtype=np.float32)
    probs[..., 0] = 1.0
    probs[:, 0, 1, 2] = (1.0 - q, 0.0, q)
    return S, walls, goal, probs


@pytest.mark.parametrize("T", [1, 2, 4, 5, 6, 37, 100])
def test_closed_form_pins_truncation(T):
    from merlin import _native as nat

    q = 0.25  # exact in float32, so the normalised row is (0.75, 0, 0.25) exactly
    S, walls, goal, probs = hand_map(q)
    want = corridor_closed_form(q, T)
    success, ret, steps, _ = nat.policy_chain_host(walls, goal, probs, S, T)
    cells = (np.array(HAND_WALLS)[:, None] >> np.arange(S)) & 1
    for name, got, ref in (("host", (success, ret, steps), None),
                           ("numpy", None, chain_ref(cells[None], goal, probs, T))):
        if ref is not None:
            got = (ref["success"], ref["ret"], ref["steps"])
        for j in range(4):  # dir j needs j left turns to face the goal: 1 -> 0, 2 -> 1 -> 0, 3 -> 2 -> 1 -> 0
            for k in range(3):
                tol = TOL * T if k == 2 else TOL
                assert abs(got[k][0, j, 1, 2] - want[k, j]) <= tol, (name, j, k)
    # the facing pose arrives at action 1 + 4 k only: one action short of the next arrival changes nothing
    if T in (4, 5):
        assert success[0, 0, 1, 2] == (q if T == 4 else q + q * (1 - q))
    assert (success[0, :, 1, 1] == 0).all() and (steps[0, :, 1, 3] == T).all()


def test_easy_5_goal_on_the_border():
    """easy at size 5: the goal replaces the border wall's corner, which no cell faces."""
    from merlin import _native as nat

    cells, walls, goal, start = _maps("easy", 5)
    probs = prob_fields("easy", 5, M9)["dirichlet"][0]
    free = np.broadcast_to((cells != 1)[:, None], (M9, 4, 5, 5))
    for T in horizons(5):
        success, ret, steps, disc = nat.policy_chain_host(walls, goal, probs, 5, T)
        assert (success[free] == 0).all() and (ret[free] == 0).all() and (disc[free] == 0).all()
        assert (steps[free] == T).all()
        st = start.copy()
        st[:, 3] = 0
        vis, hit = nat.policy_occupancy_host(walls, goal, probs, st, 5, T)
        assert (hit == 0).all() and np.abs(vis.sum((1, 2, 3)) - T).max() <= TOL * T


def test_invalid_start_pose_gives_nan_rows():
    from merlin import _native as nat

    size = 11
    cells, walls, goal, start = (a[:4] for a in _maps("mediumhard", size))
    wy, wx = np.argwhere(cells[1, 1:-1, 1:-1] == 1)[0] + 1
    pose = start.copy()
    pose[:, 3] = 0
    pose[1] = (wx, wy, 0, 0)
    pose[2] = (size, 3, 1, 0)
    probs = prob_fields("mediumhard", size, M9)["dirichlet"][0][:4]
    vis, hit = nat.policy_occupancy_host(walls, goal, probs, pose, size, 37)
    for i in (1, 2):
        assert np.isnan(vis[i]).all() and np.isnan(hit[i]).all()
    good = [0, 3]
    v2, h2 = nat.policy_occupancy_host(walls[good], goal[good], probs[good], pose[good], size, 37)
    assert np.array_equal(vis[good], v2) and np.array_equal(hit[good], h2) and np.isfinite(v2).all()
    pose[3, 2] = 4
    assert np.isnan(nat.policy_occupancy_host(walls, goal, probs, pose, size, 37)[1][3]).all()


def test_sampled_field_by_hand():
    from merlin.sampled_field import SampledField, sampled_field_from_probs

    copies, q, T, gamma = 3, 0.25, 5, 0.9
    S, walls, goal, probs = hand_map(q, copies)
    value = torch.full((copies, 4, S, S), 0.5, dtype=torch.float32)
    f = sampled_field_from_probs(torch.from_numpy(walls.astype(np.int64)).to(torch.int32), torch.from_numpy(goal),
                                 torch.from_numpy(probs), value, S, T, gamma=gamma)
    assert isinstance(f, SampledField) and int(f.free.sum()) == copies * 12 and f.max_steps == T
    for (x, y, d), dist in HAND_DIST.items():
        assert (f.dist[:, d, y, x] == dist).all()
    for t in (f.success, f.ret, f.steps, f.disc):
        assert t.dtype == torch.float64 and torch.isnan(t[~f.free]).all() and torch.isfinite(t[f.free]).all()
    # by hand, T = 5: dir j of (2, 1) arrives at action j + 1 with probability q, and dir 0 again at action 5 with
    # q (1 - q); the eight poses of (1, 1) and (3, 1) turn for ever
    r = [None] + [1.0 - 0.9 * (t / 5.0) for t in range(1, 6)]
    hand = {0: (q + q * (1 - q), q * r[1] + q * (1 - q) * r[5], q * 1 + q * (1 - q) * 5,
                q * r[1] + q * (1 - q) * gamma ** 4 * r[5])}
    for j in (1, 2, 3):
        hand[j] = (q, q * r[j + 1], q * (j + 1), q * gamma ** j * r[j + 1])
    for j, (s, rt, n, dc) in hand.items():
        n = n + T * (1.0 - s)
        for got, want in ((f.success, s), (f.ret, rt), (f.steps, n), (f.disc, dc)):
            assert (got[:, j, 1, 2] - want).abs().max() <= 1e-12, j
    # solvable within 5: every free pose but (3, 1, 0), whose dist is 6 -> 11 per map, 4 of them ever arrive
    opt = {p: float(np.float32(1.0 - 0.9 * (d / 5.0))) for p, d in HAND_DIST.items() if d <= 5}
    want = {"success_rate": sum(h[0] for h in hand.values()) / 11,
            "expected_return": sum(h[1] for h in hand.values()) / 11,
            "expected_steps": (sum(h[2] + T * (1.0 - h[0]) for h in hand.values()) + 7 * T) / 11,
            "return_regret": (sum(opt.values()) - sum(h[1] for h in hand.values())) / 11,
            "value_rmse_sampled": ((sum((0.5 - h[3]) ** 2 for h in hand.values()) + 7 * 0.25) / 11) ** 0.5}
    got = f.metrics()
    assert (got["n_maps"], got["n_free"], got["n_solvable"], got["max_steps"]) == (copies, 36, 33, T)
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
        assert all(abs(p - v) <= 1e-12 for p in got["per_map"][k]), k
    assert got["per_map"]["n_solvable"] == [11] * copies

    agent = torch.tensor([[2, 1, 0, 0], [2, 1, 3, 0], [1, 1, 1, 0]], dtype=torch.int32)
    s, rt, n = f.at(agent)
    assert s.dtype == torch.float64
    assert abs(float(s[0]) - hand[0][0]) <= 1e-12 and abs(float(s[1]) - q) <= 1e-12 and float(s[2]) == 0.0
    assert abs(float(rt[1]) - hand[3][1]) <= 1e-12 and float(rt[2]) == 0.0 and float(n[2]) == T
    vis, hit = f.occupancy(agent)
    assert vis.shape == (copies, 4, S, S) and hit.shape == (copies, T)
    assert (hit.sum(1) - s).abs().max() <= 1e-12 and (vis.sum((1, 2, 3)) - n).abs().max() <= 1e-12
    assert hit[0].tolist() == [q, 0.0, 0.0, 0.0, q * (1 - q)]
    off = f.at(torch.tensor([[5, 1, 0, 0], [0, 0, 0, 0], [2, 1, 4, 0]], dtype=torch.int32))
    assert all(torch.isnan(t).all() for t in off)
    with pytest.raises(ValueError):
        f.at(agent[:2])


def test_policies_without_probabilities_are_refused():
    from merlin import CNNActorCritic, MLPActorCritic, SampledField, sampled_field, sampled_field_for_seeds  # noqa: F401
    from merlin import sampled_field_from_probs  # noqa: F401

    walls = torch.tensor([HAND_WALLS], dtype=torch.int32)
    goal = torch.tensor([HAND_GOAL], dtype=torch.int32)
    with pytest.raises(ValueError):
        sampled_field(MLPActorCritic(9408, 3), walls, goal, 5, 20)
    with pytest.raises(ValueError):
        sampled_field(object(), walls, goal, 5, 20)
    with pytest.raises(ValueError):
        CNNActorCritic((56, 56, 3), 4).probs_codes(torch.zeros((1, 8), dtype=torch.int32))


def test_bad_probabilities_are_refused():
    """The wrappers' one reduction: a free pose's row that is negative, non-finite or sums to zero raises; the same
    values on a wall pose are ignored."""
    from merlin import _native as nat
    from merlin.sampled_field import sampled_field_from_probs

    S, walls, goal, probs = hand_map(0.25)
    agent = np.array([[2, 1, 0, 0]], dtype=np.int32)
    for bad in ((-0.5, 1.0, 0.5), (0.0, 0.0, 0.0), (np.nan, 0.5, 0.5), (np.inf, 0.0, 0.0)):
        p = probs.copy()
        p[0, 2, 1, 1] = bad
        with pytest.raises(nat.MerlinNativeError):
            nat.policy_chain_host(walls, goal, p, S, 5)
        with pytest.raises(nat.MerlinNativeError):
            nat.policy_occupancy_host(walls, goal, p, agent, S, 5)
        with pytest.raises(nat.MerlinNativeError):
            sampled_field_from_probs(torch.from_numpy(walls.astype(np.int64)).to(torch.int32), torch.from_numpy(goal),
                                     torch.from_numpy(p), torch.zeros((1, 4, S, S)), S, 5)
        p = probs.copy()
        p[0, 2, 0, 0] = bad  # a wall pose
        ok = nat.policy_chain_host(walls, goal, p, S, 5)
        assert np.array_equal(ok[0], nat.policy_chain_host(walls, goal, probs, S, 5)[0], equal_nan=True)
    with pytest.raises(nat.MerlinNativeError):
        nat.policy_chain_host(walls, goal, probs, S, 5, outputs=())
    with pytest.raises(nat.MerlinNativeError):
        nat.policy_chain_host(walls, goal, probs, S, 5, outputs=("success", "visits"))


def test_argument_checks():
    """Size 4 and 33, horizon 0 and 16385, a negative count, a null input and all outputs null return MERLIN_E_INVALID
    from all four entries before any device call; zero maps are a no-op; the ABI version stays 3."""
    from merlin import _native as nat

    L = nat.lib()
    names = ("merlin_policy_chain", "merlin_policy_chain_host", "merlin_policy_occupancy", "merlin_policy_occupancy_host")
    for s in names:
        assert s in nat.EXPORTED_SYMBOLS and getattr(L, s).argtypes is not None
    assert L.merlin_version() == nat.ABI_VERSION == 3
    vp = C.c_void_p
    walls = np.full((2, 8), 0xFF, dtype=np.uint32)
    goal = np.ones((2, 2), dtype=np.int32)
    probs = np.full((2, 4, 8, 8, 3), 0.25, dtype=np.float32)
    agent = np.ones((2, 4), dtype=np.int32)
    out = np.full((2, 4, 8, 8), 77.0, dtype=np.float64)
    w, g, p, a, o = (t.ctypes.data_as(vp) for t in (walls, goal, probs, agent, out))
    inv = 1  # MERLIN_E_INVALID

    def chain(w_, g_, p_, n, size, T, outs=(o, None, None, None)):
        return (L.merlin_policy_chain_host(w_, g_, p_, n, size, T, 0.99, *outs),
                L.merlin_policy_chain(w_, g_, p_, n, size, T, 0.99, *outs, None))

    def occ(w_, g_, p_, a_, n, size, T, outs=(o, None)):
        return (L.merlin_policy_occupancy_host(w_, g_, p_, a_, n, size, T, *outs),
                L.merlin_policy_occupancy(w_, g_, p_, a_, n, size, T, *outs, None))

    for size, T, n in ((4, 10, 2), (33, 10, 2), (8, 0, 2), (8, 16385, 2), (8, -1, 2), (8, 10, -1)):
        assert chain(w, g, p, n, size, T) == (inv, inv), (size, T, n)
        assert occ(w, g, p, a, n, size, T) == (inv, inv), (size, T, n)
    for args in ((None, g, p), (w, None, p), (w, g, None)):
        assert chain(*args, 2, 8, 10) == (inv, inv)
        assert occ(*args, a, 2, 8, 10) == (inv, inv)
    assert occ(w, g, p, None, 2, 8, 10) == (inv, inv)
    assert chain(w, g, p, 2, 8, 10, outs=(None,) * 4) == (inv, inv)
    assert occ(w, g, p, a, 2, 8, 10, outs=(None, None)) == (inv, inv)
    assert chain(None, None, None, 0, 8, 10, outs=(None,) * 4) == (0, 0)
    assert occ(None, None, None, None, 0, 8, 10, outs=(None, None)) == (0, 0)
    assert (out == 77.0).all()
    assert L.merlin_policy_chain_host(w, g, p, 2, 8, 16384, 0.99, None, None, o, None) == 0  # the longest horizon
