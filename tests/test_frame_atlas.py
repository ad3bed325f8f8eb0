"""CPU: the frame atlas (merlin_frame_atlas, the host-built tiles full-grid frames are made of) against the numpy
restatement of minigrid's render_tile (oracle/tiles.py), byte for byte."""
import numpy as np
import pytest

import tiles

OBJ = (None, "wall", "goal")


def atlas_keys():
    """(atlas index, object id, agent_dir or None, highlighted) of all 22 tiles, in the header's order."""
    keys = []
    for hl in (0, 1):
        for obj in (0, 1, 2):
            keys.append((obj + 3 * hl, obj, None, bool(hl)))
    for on_goal in (0, 1):
        for d in range(4):
            for hl in (0, 1):
                keys.append((6 + ((on_goal * 4 + d) * 2 + hl), 2 * on_goal, d, bool(hl)))
    return keys


def test_the_order_covers_22_tiles_once():
    from merlin import _native as nat

    keys = atlas_keys()
    assert sorted(k[0] for k in keys) == list(range(22)) == list(range(nat.FRAME_TILES))
    for idx, obj, d, hl in keys:
        assert nat.frame_tile_index(obj, d, hl) == idx


@pytest.mark.parametrize("ts", [5, 8, 32])  # odd and small, the observation's, minigrid's default
def test_frame_atlas_equals_render_tile(ts):
    from merlin import _native as nat

    a = nat.frame_atlas(ts)
    assert a.shape == (22, ts, ts, 3) and a.dtype == np.uint8
    for idx, obj, d, hl in atlas_keys():
        want = tiles.render_tile(OBJ[obj], d, hl, ts)
        assert (a[idx] == want).all(), (ts, idx, obj, d, hl)
    # a second call serves the cached atlas: the same bytes
    assert (nat.frame_atlas(ts) == a).all()


def test_frame_atlas_contains_the_observation_atlas():
    """The 5 tiles of the 56x56 observation (dark empty, lit empty / wall / goal, the agent facing up) are the
    frame atlas's plain empty tile, its three highlighted agent-less tiles and its highlighted dir-3 agent tile."""
    from merlin import _native as nat

    a, five = nat.frame_atlas(8), nat.tile_atlas()
    assert (a[0] == five[0]).all()
    for obj in range(3):
        assert (a[nat.frame_tile_index(obj, None, True)] == five[1 + obj]).all()
    assert (a[nat.frame_tile_index(0, 3, True)] == five[4]).all()


@pytest.mark.parametrize("ts", [3, 33])
def test_unsupported_tile_sizes_are_refused(ts):
    from merlin import _native as nat

    with pytest.raises(nat.MerlinNativeError) as e:
        nat.frame_atlas(ts)
    assert e.value.code == nat.E_INVALID
