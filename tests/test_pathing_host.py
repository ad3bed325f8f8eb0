"""CPU: the library's host restatement of the shortest-path solver (merlin_shortest_paths_host) against a forward
breadth-first search written from the step rule (tests/pathing_ref.py), its distance field against the Bellman
conditions, the path metrics on hand-made episodes and the entry points' argument checks.  The kernel itself is compared
with both in tests/test_gpu_pathing.py."""
import ctypes as C
import math

import numpy as np
import pytest

from pathing_ref import CASES, IDS, SEED0, bfs, oracle_maps


def seeds_for(size, n=130):
    return range(SEED0, SEED0 + (32 if size >= 31 else n))  # the Python search stays at a few seconds


@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_host_dist_equals_forward_bfs(oracle, diff, size):
    from merlin import _native as nat

    cells, walls, goal, agent = oracle_maps(oracle, diff, size, seeds_for(size))
    want = np.array([bfs(cells[i], agent[i, :2], agent[i, 2], goal[i]) for i in range(len(cells))], dtype=np.int32)
    dist = nat.shortest_paths_host(walls, goal, agent, size)
    assert dist.dtype == np.int32 and (dist == want).all(), np.flatnonzero(dist != want)
    d2, field = nat.shortest_paths_host(walls, goal, agent, size, field=True)
    assert (d2 == dist).all()
    q = np.arange(len(cells))
    assert (field[q, agent[:, 2], agent[:, 1], agent[:, 0]] == dist).all()


def bellman_expected(field, cells, goal):
    """What the Bellman conditions give at every pose from the field's own values: 1 where the front cell is the goal,
    otherwise 1 + the least non-negative value among the successors that exist (forward only into a free cell of the
    grid), -1 where there is none or the cell is a wall."""
    n, _, S, _ = field.shape
    free = cells != 1
    ys, xs = np.mgrid[0:S, 0:S]
    big = np.int64(1 << 30)
    out = np.empty(field.shape, dtype=np.int64)
    f = field.astype(np.int64)
    for d, (dx, dy) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
        fx, fy = xs + dx, ys + dy
        inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
        fxc, fyc = fx.clip(0, S - 1), fy.clip(0, S - 1)
        fwd = np.where(inside[None] & free[:, fyc, fxc], f[:, d][:, fyc, fxc], -1)
        succ = np.stack([fwd, f[:, (d + 3) & 3], f[:, (d + 1) & 3]])
        best = np.where(succ >= 0, succ, big).min(0)
        front_goal = (fx[None] == goal[:, 0, None, None]) & (fy[None] == goal[:, 1, None, None])
        v = np.where(front_goal, 1, np.where(best < big, best + 1, -1))
        out[:, d] = np.where(free, v, -1)
    return out


@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_host_field_satisfies_bellman(oracle, diff, size):
    """With unit costs the conditions have one solution, so they pin the whole field."""
    from merlin import _native as nat

    cells, walls, goal, agent = oracle_maps(oracle, diff, size, range(SEED0, SEED0 + 130))
    _, field = nat.shortest_paths_host(walls, goal, agent, size, field=True)
    assert field.dtype == np.int16 and field.shape == (130, 4, size, size)
    want = bellman_expected(field, cells, goal)
    assert (field == want).all(), np.argwhere(field != want)[:5]
    assert (field >= 0).any() or (diff, size) == ("easy", 5)


def test_conditions_the_gpu_tests_rely_on(oracle):
    """The counts tests/test_gpu_pathing.py asserts on the kernel, here on the host solver and the forward search."""
    from merlin import _native as nat
    from merlin.pathing import optimal_reward

    seeds = range(SEED0, SEED0 + 130)
    cells, walls, goal, agent = oracle_maps(oracle, "easy", 6, seeds)
    on_goal = (agent[:, :2] == goal).all(1)
    dist = nat.shortest_paths_host(walls, goal, agent, 6)
    assert on_goal.sum() == 10 and set(dist[on_goal]) <= {4, 5}
    cells, walls, goal, agent = oracle_maps(oracle, "easy", 5, seeds)
    dist = nat.shortest_paths_host(walls, goal, agent, 5)
    assert (goal == 0).all() and (dist == -1).all() and (optimal_reward(dist, 100) == 0).all()
    cells, walls, goal, agent = oracle_maps(oracle, "hard", 17, seeds)
    dist = nat.shortest_paths_host(walls, goal, agent, 17)
    assert ((dist > 20).sum(), ((dist >= 1) & (dist <= 20)).sum(), (dist == 20).sum()) == (38, 92, 7)
    assert (optimal_reward(dist, 20)[dist == 20] == np.float32(0.1)).all()


def test_optimal_reward():
    import torch

    from merlin.pathing import optimal_reward

    d = np.array([-1, 0, 1, 7, 20, 21], dtype=np.int32)
    r = optimal_reward(d, 20)
    assert r.dtype == np.float32
    want = [0.0, 0.0, np.float32(1.0 - 0.9 * (1 / 20)), np.float32(1.0 - 0.9 * (7 / 20)), np.float32(0.1), 0.0]
    assert r.tolist() == [float(w) for w in want]
    t = optimal_reward(torch.from_numpy(d), 20)
    assert t.dtype == torch.float32 and (t.numpy() == r).all()
    # every dist of a default 32x32 episode: the same bits from both forms
    d = np.arange(0, 4100, dtype=np.int32)
    assert (optimal_reward(torch.from_numpy(d), 4096).numpy() == optimal_reward(d, 4096)).all()


def test_path_metrics():
    from merlin.pathing import optimal_reward, path_metrics

    ms = 40
    opt = np.array([4, 10, 40, 7])
    m = path_metrics(optimal_reward(opt, ms), opt, opt, ms)  # all optimal
    assert m["n_tasks"] == m["n_solvable"] == 4
    assert m["spl"] == 1.0 and m["regret_mean"] == 0.0 and m["reward_ratio"] == 1.0 and m["success_rate"] == 1.0
    assert m["excess_steps_mean"] == 0.0
    assert m["per_task"]["opt_rewards"][2] == np.float32(0.1)  # dist == max_steps is solvable
    # the same rewards as f64 episode returns (the env's accumulator) are still exactly optimal
    m = path_metrics([1.0 - 0.9 * (o / ms) for o in opt], opt, opt, ms)
    assert m["regret_mean"] == 0.0 and m["reward_ratio"] == 1.0
    # a failure contributes 0, an episode of twice the optimum 0.5; unsolvable tasks (-1, beyond the horizon) are
    # left out and counted
    opt = np.array([4, 10, 5, -1, 41])
    steps = np.array([4, 20, 40, 40, 40])
    rew = np.array([optimal_reward(4, ms), optimal_reward(20, ms), 0.0, 0.0, 0.0], dtype=np.float64)
    m = path_metrics(rew, steps, opt, ms)
    assert (m["n_tasks"], m["n_solvable"]) == (5, 3)
    assert m["per_task"]["solvable"].tolist() == [True, True, True, False, False]
    assert m["per_task"]["spl"].tolist() == [1.0, 0.5, 0.0, 0.0, 0.0]
    assert m["spl"] == pytest.approx(0.5) and m["success_rate"] == pytest.approx(2 / 3)
    assert m["excess_steps_mean"] == 5.0
    o = optimal_reward(opt[:3], ms).astype(np.float64)
    assert m["optimal_reward_mean"] == pytest.approx(o.mean())
    assert m["regret_mean"] == pytest.approx((o - rew[:3]).mean())
    assert m["reward_ratio"] == pytest.approx((rew[:3] / o).mean())
    # no solvable task: nan, no exception
    m = path_metrics([0.0, 0.0], [40, 40], [-1, 99], ms)
    assert (m["n_tasks"], m["n_solvable"]) == (2, 0)
    for k in ("success_rate", "spl", "excess_steps_mean", "optimal_reward_mean", "reward_ratio", "regret_mean"):
        assert math.isnan(m[k]), k
    with pytest.raises(ValueError):
        path_metrics([0.0], [1, 2], [1], ms)


def test_evaluate_efficiency_refuses_shaped_rewards():
    from merlin.pathing import evaluate_efficiency

    for flag in ("stuck_penalty", "exploration_bonus"):
        with pytest.raises(ValueError, match=flag):
            evaluate_efficiency(None, [1, 2], **{flag: True})


def test_argument_checks():
    """Size 4, size 33 and null pointers return MERLIN_E_INVALID from all three entries, before any device call."""
    from merlin import _native as nat

    L = nat.lib()
    for s in ("merlin_shortest_paths", "merlin_env_optimal_steps", "merlin_shortest_paths_host"):
        assert s in nat.EXPORTED_SYMBOLS and getattr(L, s).argtypes is not None
    assert L.merlin_version() == nat.ABI_VERSION == 3
    walls = np.full((2, 8), 0xFF, dtype=np.uint32)
    goal = np.ones((2, 2), dtype=np.int32)
    agent = np.ones((2, 4), dtype=np.int32)
    dist = np.full(2, 77, dtype=np.int32)
    vp = C.c_void_p
    w, g, a, d = (x.ctypes.data_as(vp) for x in (walls, goal, agent, dist))
    for size in (4, 33):
        assert L.merlin_shortest_paths_host(w, g, a, 2, size, d, None) == nat.E_INVALID
        assert L.merlin_shortest_paths(w, g, a, None, 2, size, d, None, None) == nat.E_INVALID
    assert L.merlin_shortest_paths_host(w, g, a, -1, 8, d, None) == nat.E_INVALID
    assert L.merlin_shortest_paths(w, g, a, None, -1, 8, d, None, None) == nat.E_INVALID
    for args in ((None, g, a, 2, 8, d, None), (w, None, a, 2, 8, d, None), (w, g, None, 2, 8, d, None),
                 (w, g, a, 2, 8, None, None)):
        assert L.merlin_shortest_paths_host(*args) == nat.E_INVALID
        assert L.merlin_shortest_paths(*args[:3], None, *args[3:], None) == nat.E_INVALID
    assert L.merlin_env_optimal_steps(None, d, None, None) == nat.E_INVALID
    assert (dist == 77).all()
    # n = 0 is a no-op, null pointers and all
    assert L.merlin_shortest_paths_host(None, None, None, 0, 8, None, None) == nat.MERLIN_OK
    assert L.merlin_shortest_paths(None, None, None, None, 0, 8, None, None, None) == nat.MERLIN_OK
    with pytest.raises(nat.MerlinNativeError):
        nat.shortest_paths_host(walls[:, :4], goal, agent, 4)
    # poses that are no free cell of the grid: -1, on a map where every other pose has an answer
    walls = np.zeros((6, 8), dtype=np.uint32)
    walls[:, 3] = 1 << 5
    goal = np.tile(np.array([[4, 4]], dtype=np.int32), (6, 1))
    agent = np.array([[1, 1, 0, 0], [-1, 1, 0, 0], [1, 8, 0, 0], [5, 3, 0, 0], [1, 1, 4, 0], [1, 1, -1, 0]],
                     dtype=np.int32)
    assert nat.shortest_paths_host(walls, goal, agent, 8).tolist() == [7, -1, -1, -1, -1, -1]
    goal[:] = (8, 4)  # a goal outside the grid: nothing reaches it
    d, f = nat.shortest_paths_host(walls, goal, agent, 8, field=True)
    assert (d == -1).all() and (f == -1).all()
