"""CPU: what merlin/pose_fields.py and merlin._native's map helpers give the three map analyses -- the distance
field's host route, the ratio reductions at their empty edge, the shared argument checks -- on the 5x5 hand map
(tests/hand_map.py)."""
import numpy as np
import pytest
import torch

from hand_map import HAND_DIST, HAND_GOAL, HAND_WALLS


def test_distance_field_on_cpu_is_the_host_solver():
    from merlin import _native as nat
    from merlin.pose_fields import distance_field

    walls = np.array([HAND_WALLS, HAND_WALLS], dtype=np.uint32)
    goal = np.array([HAND_GOAL, (9, 9)], dtype=np.int32)  # the second map's goal is off the grid: no pose reaches it
    got = distance_field(torch.from_numpy(walls.astype(np.int32)), torch.from_numpy(goal), 5)
    _, want = nat.shortest_paths_host(walls, goal, np.zeros((2, 4), dtype=np.int32), 5, field=True)
    assert got.dtype == torch.int16 and got.shape == (2, 4, 5, 5)
    assert (got.numpy() == want).all()
    assert all(got[0, d, y, x] == v for (x, y, d), v in HAND_DIST.items())
    assert (got[0] >= 1).sum() == len(HAND_DIST) and (got[1] == -1).all()


def test_moved_names_stay_importable():
    from merlin import pose_fields
    from merlin.policy_field import PolicyField, free_cells, free_poses
    from merlin.sampled_field import SampledField

    assert free_cells is pose_fields.free_cells and free_poses is pose_fields.free_poses
    assert issubclass(PolicyField, pose_fields.PoseField) and issubclass(SampledField, pose_fields.PoseField)


def test_ratios_are_nan_without_a_denominator():
    from merlin.pose_fields import ratio

    v = torch.tensor([[[[1.0, 2.0]]], [[[4.0, 8.0]]]], dtype=torch.float64)
    den = torch.tensor([[[[True, True]]], [[[False, False]]]])
    assert float(ratio(v, den)) == 7.5
    pm = ratio(v, den, per_map=True)
    assert pm.dtype == torch.float64 and pm.shape == (2,) and pm[0] == 1.5 and torch.isnan(pm[1])
    assert np.isnan(float(ratio(v, torch.zeros_like(den))))


def test_device_map_checks():
    from merlin import _native as nat

    walls = torch.zeros((3, 5), dtype=torch.int32)
    goal = torch.zeros((3, 2), dtype=torch.int32)
    agent = torch.zeros((2, 4), dtype=torch.int32)
    index = torch.tensor([2, 0], dtype=torch.int32)
    assert nat._device_maps("t", walls, goal, 5) == (5, 3, 3)
    assert nat._device_maps("t", walls, goal, 5, agent) == (5, 3, 2)
    assert nat._device_maps("t", walls, None, 5, agent, index, goal_optional=True) == (5, 3, 2)
    with pytest.raises(nat.MerlinNativeError, match=r"t: map_index outside \[0, M\)"):
        nat._device_maps("t", walls, goal, 5, agent, index + 1)
    with pytest.raises(nat.MerlinNativeError):
        nat._device_maps("t", walls, goal, 5, agent, index - 1)
    for bad in (dict(walls=walls.long()), dict(size=6), dict(goal=goal[:2]), dict(goal=None), dict(agent=agent[:, :3]),
                dict(agent=torch.zeros((4, 4), dtype=torch.int32)), dict(map_index=index.long()),
                dict(map_index=index[:1])):
        args = dict(walls=walls, goal=goal, size=5, agent=agent, map_index=bad.get("map_index"))
        args.update(bad)
        with pytest.raises(AssertionError):
            nat._device_maps("t", **args)


def test_host_map_conversion():
    from merlin import _native as nat

    walls = np.array([HAND_WALLS], dtype=np.int64)[:, ::1]
    S, M, w, g, a = nat._host_maps(5, walls, [HAND_GOAL], (np.zeros((1, 4), dtype=np.int64), "int32", (4,)))
    assert (S, M) == (5, 1) and w.dtype == np.uint32 and g.dtype == np.int32 and a.dtype == np.int32
    assert all(x.flags.c_contiguous for x in (w, g, a)) and (w == walls).all() and g.shape == (1, 2)
    with pytest.raises(AssertionError):
        nat._host_maps(5, walls, [HAND_GOAL], (np.zeros((2, 4)), "int32", (4,)))
    with pytest.raises(AssertionError):
        nat._host_maps(4, walls, [HAND_GOAL])
    assert nat.np_ptr(None) is None and nat.np_ptr(w).value == w.ctypes.data
