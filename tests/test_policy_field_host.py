"""CPU: the library's host restatement of the policy search (merlin_policy_paths_host: a forward walk per pose with
memoisation and cycle marks) against the tests' own walk (tests/policy_field_ref.py: the step rule applied action by
action, nothing remembered), at every grid size of test_gpu_env_sizes' matrix on the CPU oracle's maps; the identity
steps == dist under a shortest-path policy; and merlin.policy_field's torch side -- free_poses, metrics,
predicted_episode -- on a 5x5 map small enough to work out by hand."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from hand_map import HAND_ACTIONS, HAND_DIST, HAND_GOAL, HAND_STEPS, HAND_WALLS  # noqa: F401
from policy_field_ref import CASES, IDS, SEEDS9, bouncer_field, oracle_maps, seeker_field, walk

M9 = len(SEEDS9)


@functools.lru_cache(maxsize=None)
def _maps(diff, size):
    import oracle as O

    O.build()
    return oracle_maps(O, diff, size, SEEDS9)


def random_field(size, seed, m=M9):
    """Uniform over {0, 1, 2}, with -1 and 3 in a few poses."""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 3, size=(m, 4, size, size)).astype(np.int8)
    bad = rs.rand(m, 4, size, size) < 0.02
    a[bad] = rs.choice([-1, 3], size=int(bad.sum())).astype(np.int8)
    return a


def oracle_field(nat, walls, goal, size):
    """A shortest-path action at every pose: merlin.pathing.oracle_actions on the host distance field."""
    from merlin.pathing import oracle_actions

    m = walls.shape[0]
    _, dist = nat.shortest_paths_host(walls, goal, np.zeros((m, 4), dtype=np.int32), size, field=True)
    d, y, x = np.meshgrid(np.arange(4), np.arange(size), np.arange(size), indexing="ij")
    poses = torch.from_numpy(np.stack([x, y, d, np.zeros_like(x)], -1).reshape(-1, 4).astype(np.int32))
    n = poses.shape[0]
    out = np.empty((m, 4, size, size), dtype=np.int8)
    wt, gt, ft = torch.from_numpy(walls.astype(np.int32)), torch.from_numpy(goal), torch.from_numpy(dist)
    for i in range(m):
        a = oracle_actions(ft[i:i + 1].expand(n, -1, -1, -1), wt[i:i + 1].expand(n, -1), gt[i:i + 1].expand(n, -1),
                           poses)
        out[i] = a.numpy().astype(np.int8).reshape(4, size, size)
    return out, dist


@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_host_equals_walk(diff, size):
    from merlin import _native as nat

    cells, walls, goal, _ = _maps(diff, size)
    fields = {"random": random_field(size, 7 * size + len(diff)),
              "bouncer": np.stack([bouncer_field(c) for c in cells]),
              "seeker": np.stack([seeker_field(c, g) for c, g in zip(cells, goal)]),
              "forward": np.full((M9, 4, size, size), 2, dtype=np.int8)}
    assert ((fields["random"] == -1).sum() > 0 and (fields["random"] == 3).sum() > 0) or size == 5
    for name, a in fields.items():
        got = nat.policy_paths_host(walls, goal, a, size)
        assert got.dtype == np.int16 and got.shape == (M9, 4, size, size)
        want = walk(cells, goal, a)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, bad[:5])
        assert (got[np.broadcast_to((cells == 1)[:, None], got.shape)] == -1).all()


@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_oracle_policy_gives_dist_and_left_gives_nothing(diff, size):
    """Under a shortest-path action at every pose steps == dist everywhere, the goal cell's poses included; turning
    left for ever terminates nowhere."""
    from merlin import _native as nat

    cells, walls, goal, _ = _maps(diff, size)
    a, dist = oracle_field(nat, walls, goal, size)
    steps = nat.policy_paths_host(walls, goal, a, size)
    assert (steps == dist).all(), np.argwhere(steps != dist)[:5]
    assert (steps == walk(cells, goal, a)).all()
    gx, gy = goal[:, 0], goal[:, 1]
    if diff != "easy" or size != 5:  # easy 5: the goal is the border's corner, which no cell faces
        on_goal = steps[np.arange(M9), :, gy, gx]
        # leave, turn round twice, come back: 4, plus up to two turns to face a free neighbour (-1: there is none)
        assert (((on_goal >= 4) & (on_goal <= 6)) | (on_goal == -1)).all() and (on_goal >= 4).any(), on_goal
    left = nat.policy_paths_host(walls, goal, np.zeros_like(a), size)
    assert (left == -1).all()


def test_pose_in_front_of_the_goal_stays_at_one():
    """The forward-acting free pose in front of the goal has steps 1 although the goal-cell pose behind it, which an
    ordinary forward edge would hang it under, has finite steps of its own: present in the maps (by construction: a
    shortest-path policy, under which every goal-cell pose is finite), and answered with 1."""
    from merlin import _native as nat

    vec = ((1, 0), (0, 1), (-1, 0), (0, -1))
    seen = 0
    for diff, size in (("medium", 15), ("hard", 17), ("hardest", 9)):
        cells, walls, goal, _ = _maps(diff, size)
        a, _ = oracle_field(nat, walls, goal, size)
        steps = nat.policy_paths_host(walls, goal, a, size)
        for m in range(M9):
            gx, gy = int(goal[m, 0]), int(goal[m, 1])
            for d in range(4):
                fx, fy = gx - vec[d][0], gy - vec[d][1]
                if not (0 <= fx < size and 0 <= fy < size) or cells[m, fy, fx] == 1:
                    continue
                assert a[m, d, fy, fx] == 2            # in front of the goal the shortest path is forward
                assert steps[m, d, gy, gx] >= 4        # the pose that stands on the goal, same direction: finite
                assert steps[m, d, fy, fx] == 1
                seen += 1
    assert seen >= 27


@pytest.mark.parametrize("diff,size", [("mediumhard", 6), ("hard", 17), ("hardest", 32)])
def test_free_poses_order_and_counts(diff, size):
    from merlin.policy_field import free_poses

    cells, walls, _, _ = _maps(diff, size)
    agent, index = free_poses(torch.from_numpy(walls.astype(np.int32)), size)
    assert agent.dtype == torch.int32 and index.dtype == torch.int32 and agent.shape == (len(index), 4)
    want = [(m, d, y, x) for m in range(M9) for d in range(4) for y in range(size) for x in range(size)
            if cells[m, y, x] != 1]
    assert len(want) == 4 * int((cells != 1).sum()) == len(index)
    got = np.stack([index.numpy(), agent[:, 2].numpy(), agent[:, 1].numpy(), agent[:, 0].numpy()], 1)
    assert (got == np.array(want)).all() and (agent[:, 3] == 0).all()


def test_metrics_and_predicted_episode_by_hand():
    from merlin.policy_field import field_from_actions

    copies, S, ms, gamma = 3, 5, 5, 0.99
    walls = torch.tensor([HAND_WALLS] * copies, dtype=torch.int32)
    goal = torch.tensor([HAND_GOAL] * copies, dtype=torch.int32)
    action = torch.full((copies, 4, S, S), 2, dtype=torch.int8)  # wall poses: anything; the field sets them to -1
    value = torch.full((copies, 4, S, S), 0.5, dtype=torch.float32)
    for (x, y, d), a in HAND_ACTIONS.items():
        action[:, d, y, x] = a
    f = field_from_actions(walls, goal, action, value, S)
    assert int(f.free.sum()) == copies * 12 and (f.action[~f.free] == -1).all()
    for (x, y, d), s in HAND_STEPS.items():
        assert (f.steps[:, d, y, x] == s).all(), (x, y, d)
        assert (f.dist[:, d, y, x] == HAND_DIST[(x, y, d)]).all(), (x, y, d)
    assert (f.steps[~f.free] == -1).all() and (f.dist[~f.free] == -1).all()

    def rew(s):  # the step kernel's expression, rounded to float32
        return float(np.float32(1.0 - 0.9 * (s / 5.0)))

    solved_steps = [1, 2, 3, 4, 2, 3, 4, 5]
    se = sum((0.5 - gamma ** (s - 1) * rew(s)) ** 2 for s in solved_steps) + 3 * 0.25
    want = {"solved_rate": 8 / 11, "trapped_rate": 2 / 11, "timeout_rate": 1 / 11, "spl": 7.5 / 11,
            "excess_steps": 2 / 8, "optimal_action_rate": 7 / 11, "value_rmse": (se / 11) ** 0.5}
    got = f.metrics(ms, gamma=gamma)
    assert (got["n_maps"], got["n_free"], got["n_solvable"]) == (copies, 36, 33)
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
        if k != "value_rmse":
            assert all(abs(p - v) <= 1e-12 for p in got["per_map"][k]), k
    assert got["per_map"]["n_solvable"] == [11] * copies

    agent = torch.tensor([[1, 1, 3, 0], [1, 1, 1, 0], [3, 1, 3, 0]], dtype=torch.int32)
    st, di = f.at(agent)
    assert st.tolist() == [3, -1, 7] and di.tolist() == [3, 3, 5]
    r, n = f.predicted_episode(agent, ms)
    assert r.dtype == torch.float32 and n.dtype == torch.int64
    assert n.tolist() == [3, 5, 5] and r.tolist() == [rew(3), 0.0, 0.0]
    r, n = f.predicted_episode(agent, 7)  # the third pose arrives exactly at the horizon
    assert n.tolist() == [3, 7, 7] and r[2].item() == float(np.float32(1.0 - 0.9 * (7 / 7.0))) and r[1].item() == 0.0
    with pytest.raises(ValueError):
        f.at(agent[:2])


def test_mlp_policies_are_refused():
    from merlin.actor_critic import MLPActorCritic
    from merlin.policy_field import policy_field

    walls = torch.tensor([HAND_WALLS], dtype=torch.int32)
    with pytest.raises(ValueError):
        policy_field(MLPActorCritic(9408, 3), walls, torch.tensor([HAND_GOAL], dtype=torch.int32), 5)


def test_argument_checks():
    """Size 4, size 33, a negative count and null pointers return MERLIN_E_INVALID from all three entries before any
    device call; zero queries are a no-op."""
    from merlin import _native as nat

    L = nat.lib()
    for s in ("merlin_view_codes", "merlin_policy_paths", "merlin_policy_paths_host"):
        assert s in nat.EXPORTED_SYMBOLS and getattr(L, s).argtypes is not None
    assert L.merlin_version() == nat.ABI_VERSION == 3
    vp = C.c_void_p
    walls = np.full((2, 8), 0xFF, dtype=np.uint32)
    goal = np.ones((2, 2), dtype=np.int32)
    act = np.zeros((2, 4, 8, 8), dtype=np.int8)
    steps = np.full((2, 4, 8, 8), 77, dtype=np.int16)
    w, g, a, s = (t.ctypes.data_as(vp) for t in (walls, goal, act, steps))
    inv = 1  # MERLIN_E_INVALID
    for size in (4, 33):
        assert L.merlin_policy_paths_host(w, g, a, 2, size, s) == inv
        assert L.merlin_policy_paths(w, g, a, 2, size, s, None) == inv
        assert L.merlin_view_codes(w, g, a, None, 2, size, s, None) == inv
    assert L.merlin_policy_paths_host(w, g, a, -1, 8, s) == inv
    assert L.merlin_policy_paths(w, g, a, -1, 8, s, None) == inv and L.merlin_view_codes(w, g, a, None, -1, 8, s, None) == inv
    for args in ((None, g, a), (w, None, a), (w, g, None)):
        assert L.merlin_policy_paths_host(*args, 2, 8, s) == inv
        assert L.merlin_policy_paths(*args, 2, 8, s, None) == inv
    assert L.merlin_policy_paths_host(w, g, a, 2, 8, None) == inv and L.merlin_policy_paths(w, g, a, 2, 8, None, None) == inv
    assert L.merlin_view_codes(None, g, a, None, 2, 8, s, None) == inv
    assert L.merlin_view_codes(w, g, None, None, 2, 8, s, None) == inv
    assert L.merlin_view_codes(w, g, a, None, 2, 8, None, None) == inv
    assert L.merlin_policy_paths_host(w, g, a, 0, 8, s) == 0 and L.merlin_policy_paths(None, None, None, 0, 8, None, None) == 0
    assert L.merlin_view_codes(None, None, None, None, 0, 8, None, None) == 0
    assert (steps == 77).all()
