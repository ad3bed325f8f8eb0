"""GPU: the full-grid renderer (merlin_render_frames / merlin_env_render / merlin_env_snapshot, MerlinVecEnv.
render_frames / snapshot, MerlinEnv.render / get_frame) against tests/render_ref.py::full_render, byte for byte."""
import numpy as np
import pytest
import torch

import render_ref as RR

pytestmark = pytest.mark.gpu

DIFFS = ["easy", "medium", "mediumhard", "hard", "hardest"]


def bordered(S, extra=()):
    """cells uint8[S][S] ([y][x], 1 = wall): the border walls plus `extra` (x, y) walls."""
    c = np.zeros((S, S), dtype=np.uint8)
    c[0, :] = c[S - 1, :] = c[:, 0] = c[:, S - 1] = 1
    for x, y in extra:
        c[y, x] = 1
    return c


def rows_of(cells):
    S = cells.shape[0]
    return (cells.astype(np.uint64) << np.arange(S, dtype=np.uint64)[None, :]).sum(1).astype(np.uint32)


def state(cells, goal, pos, d):
    return {"cells": cells, "goal": goal, "pos": pos, "dir": d}


def hand_states():
    """name -> state.  Size 9 unless named otherwise."""
    walls9 = [(3, 2), (5, 5), (6, 3), (2, 6)]
    st = {}
    for d in range(4):  # all four directions, walls on every side of the agent
        st[f"dir{d}"] = state(bordered(9, walls9), (7, 7), (4, 4), d)
    st["on_goal"] = state(bordered(9, walls9), (4, 3), (4, 3), 1)
    st["corner"] = state(bordered(9), (7, 7), (1, 1), 2)  # the window overhangs the left and the top border
    st["corner_br"] = state(bordered(9), (1, 1), (7, 7), 1)  # ... the bottom and the right one
    # a wall across the whole view directly in front (process_vis sees round anything narrower): all behind it is dark
    st["wall_in_front"] = state(bordered(9, [(3, y) for y in range(1, 8)]), (7, 1), (2, 4), 0)
    st["size32"] = state(bordered(32, [(29, 30), (15, 15)]), (1, 1), (30, 30), 3)  # walls in bit 31 and row 31
    st["size5"] = state(bordered(5), (3, 3), (1, 2), 0)
    return st


def to_device(states, device):
    S = states[0]["cells"].shape[0]
    walls = torch.from_numpy(np.stack([rows_of(s["cells"]) for s in states]).view(np.int32)).to(device)
    goal = torch.tensor([s["goal"] for s in states], dtype=torch.int32, device=device)
    agent = torch.tensor([[s["pos"][0], s["pos"][1], s["dir"], 0] for s in states], dtype=torch.int32, device=device)
    return S, walls, goal, agent


def want(s, ts, hl, info=None):
    return RR.full_render(s["cells"], s["goal"], s["pos"], s["dir"], ts, hl, info=info)


def test_the_state_set_holds_every_situation():
    """A weaker set of hand-built states must not pass silently: what the cases below rely on is asserted here."""
    st = hand_states()
    info = {k: {} for k in st}
    for k, s in st.items():
        want(s, 5, True, info[k])
    assert {st[f"dir{d}"]["dir"] for d in range(4)} == {0, 1, 2, 3}
    assert st["on_goal"]["goal"] == st["on_goal"]["pos"]
    assert info["corner"]["outside"] >= 7 + 6 and info["corner_br"]["outside"] >= 7 + 6  # two borders overhung
    assert info["wall_in_front"]["dark"] >= 2  # in-grid cells inside the window that stay dark
    # ... and those dark cells really come out un-highlighted: behind the wall the plain empty tile
    img = want(st["wall_in_front"], 5, True)
    assert (img[4 * 5:5 * 5, 4 * 5:5 * 5] == RR.tile(None, None, False, 5)).all()
    assert (img[4 * 5:5 * 5, 3 * 5:4 * 5] == RR.tile("wall", None, True, 5)).all()
    c32 = st["size32"]["cells"]
    assert (rows_of(c32) >> 31).all() and rows_of(c32)[31] == 0xFFFFFFFF
    assert st["size5"]["cells"].shape == (5, 5)
    assert (5 * 5 * 5 * 5 * 3) % 16 != 0  # 5x5 at 5 px: 1,875 B, a frame that ends off a 16-B boundary


@pytest.mark.parametrize("highlight", [True, False])
@pytest.mark.parametrize("ts", [5, 8, 32])
def test_stateless_frames_of_hand_built_states(device, ts, highlight):
    from merlin import _native as nat

    st = hand_states()
    for size in (9, 32, 5):
        group = [s for s in st.values() if s["cells"].shape[0] == size]
        S, walls, goal, agent = to_device(group, device)
        got = nat.render_frames(walls, goal, agent, S, ts, highlight).cpu().numpy()  # map_index NULL, F = 1 at 32, 5
        assert got.shape == (len(group), S * ts, S * ts, 3)
        for k, s in enumerate(group):
            assert (got[k] == want(s, ts, highlight)).all(), (size, k, ts, highlight)
    assert nat.tower_errors(device) == 0


def test_map_index_permutation_with_fewer_maps_than_frames(device):
    from merlin import _native as nat

    st = hand_states()
    maps = [st["dir0"], st["corner"], st["wall_in_front"]]  # M = 3
    S, walls, goal, _ = to_device(maps, device)
    frames = [(2, (2, 4), 0), (0, (4, 4), 3), (1, (1, 1), 2), (2, (5, 4), 2), (1, (7, 7), 1), (0, (4, 4), 1),
              (1, (4, 4), 0)]  # F = 7: (map, agent position, direction)
    agent = torch.tensor([[p[0], p[1], d, 0] for _, p, d in frames], dtype=torch.int32, device=device)
    index = torch.tensor([m for m, _, _ in frames], dtype=torch.int32, device=device)
    got = nat.render_frames(walls, goal, agent, S, 8, True, map_index=index).cpu().numpy()
    for k, (m, p, d) in enumerate(frames):
        assert (got[k] == RR.full_render(maps[m]["cells"], maps[m]["goal"], p, d, 8, True)).all(), k
    with pytest.raises(nat.MerlinNativeError):  # an index past the maps is refused before the launch
        nat.render_frames(walls, goal, agent, S, 8, True, map_index=index + 1)


def test_130_frames(device):
    """More than two waves' worth of frames, not a multiple of 64, at 9x9 cells of 8 px."""
    from merlin import _native as nat

    st = hand_states()
    maps = [st["dir0"], st["corner"], st["wall_in_front"], st["on_goal"]]
    S, walls, goal, _ = to_device(maps, device)
    rs = np.random.RandomState(5)
    frames = []
    while len(frames) < 130:
        m, x, y, d = rs.randint(4), rs.randint(1, 8), rs.randint(1, 8), rs.randint(4)
        if maps[m]["cells"][y, x] == 0:
            frames.append((m, (x, y), d))
    agent = torch.tensor([[p[0], p[1], d, 0] for _, p, d in frames], dtype=torch.int32, device=device)
    index = torch.tensor([m for m, _, _ in frames], dtype=torch.int32, device=device)
    got = nat.render_frames(walls, goal, agent, S, 8, True, map_index=index).cpu().numpy()
    for k, (m, p, d) in enumerate(frames):
        assert (got[k] == RR.full_render(maps[m]["cells"], maps[m]["goal"], p, d, 8, True)).all(), k


@pytest.mark.parametrize("ts,offset", [(5, 1875), (5, 16), (8, 1), (8, 4), (8, 24), (7, 2)])
def test_unaligned_output_and_frame_tails(device, ts, offset):
    """Frames whose byte count is no multiple of 16 (5x5 at 5 px: 1,875 B) and an output that starts `offset` bytes
    into an allocation (1,875: one such frame), so that frame bases sit off every alignment: the bytes must be right
    and nothing outside the output written."""
    from merlin import _native as nat

    s5 = hand_states()["size5"]
    group = [state(s5["cells"], s5["goal"], p, d) for p, d in [((1, 2), 0), ((3, 1), 2), ((2, 2), 3), ((3, 3), 1)]]
    S, walls, goal, agent = to_device(group, device)
    fb = (S * ts) ** 2 * 3
    buf = torch.full((offset + 4 * fb + 64,), 0xAB, dtype=torch.uint8, device=device)
    out = buf[offset:offset + 4 * fb]
    nat.render_frames(walls, goal, agent, S, ts, True, out=out)
    host = buf.cpu().numpy()
    assert (host[:offset] == 0xAB).all() and (host[offset + 4 * fb:] == 0xAB).all()
    got = host[offset:offset + 4 * fb].reshape(4, S * ts, S * ts, 3)
    for k, s in enumerate(group):
        assert (got[k] == want(s, ts, True)).all(), k


def test_arguments_are_validated(device):
    from merlin import _native as nat

    S, walls, goal, agent = to_device([hand_states()["dir0"]], device)
    for size, ts in [(4, 8), (33, 8), (9, 3), (9, 33)]:
        w = torch.zeros((1, size), dtype=torch.int32, device=device)
        with pytest.raises(nat.MerlinNativeError) as e:
            nat.render_frames(w, goal, agent, size, ts, True, out=torch.empty(agent.shape[0] * (size * ts) ** 2 * 3,
                                                                             dtype=torch.uint8, device=device))
        assert e.value.code == nat.E_INVALID
    with pytest.raises(nat.MerlinNativeError):  # a non-contiguous out
        nat.render_frames(walls, goal, agent, S, 8, True,
                          out=torch.empty((1, S * 8, S * 8, 6), dtype=torch.uint8, device=device)[..., ::2])
    with pytest.raises(nat.MerlinNativeError):  # a wrong-sized one
        nat.render_frames(walls, goal, agent, S, 8, True, out=torch.empty(10, dtype=torch.uint8, device=device))


def test_a_bad_agent_is_skipped_and_flagged(device):
    """An agent outside the grid, with a direction outside 0..3 or on a wall indexes nothing: its frame shows the map
    alone, the other frames are untouched, and the device error bit is raised."""
    from merlin import _native as nat

    s = hand_states()["dir0"]
    S, walls, goal, _ = to_device([s], device)
    agents = [[4, 4, 1, 0], [9, 4, 0, 0], [4, -1, 0, 0], [4, 4, 7, 0], [0, 0, 0, 0], [1 << 30, -(1 << 30), -5, 0]]
    agent = torch.tensor(agents, dtype=torch.int32, device=device)
    index = torch.zeros(len(agents), dtype=torch.int32, device=device)
    nat.tower_errors(device, raise_on_error=False)
    got = nat.render_frames(walls, goal, agent, S, 8, True, map_index=index).cpu().numpy()
    assert (got[0] == RR.full_render(s["cells"], s["goal"], (4, 4), 1, 8, True)).all()
    bare = np.zeros((S * 8, S * 8, 3), dtype=np.uint8)
    grid = RR.grid_of(s["cells"], s["goal"])
    for j in range(S):
        for i in range(S):
            bare[j * 8:j * 8 + 8, i * 8:i * 8 + 8] = RR.tile(grid.get(i, j), None, False, 8)
    for k in range(1, len(agents)):
        assert (got[k] == bare).all(), k
    assert nat.tower_errors(device, raise_on_error=False) == nat.DEVERR_BAD_FRAME
    assert nat.tower_errors(device, raise_on_error=False) == 0


@pytest.mark.parametrize("size", [16, 17])
def test_live_envs(device, size):
    from merlin import MerlinVecEnv
    from merlin import _native as nat

    n = 70
    env = MerlinVecEnv(n, difficulty=[DIFFS[i % 5] for i in range(n)], size=size, seed=4242, device=device,
                       max_steps=9)  # short episodes: the 12 steps cross auto-resets
    env.reset()
    rs = np.random.RandomState(size)

    def check(ts):
        stt = env.get_state()
        got = env.render_frames(ts)
        assert got.shape == (n, size * ts, size * ts, 3) and got.dtype == torch.uint8 and got.device.type == "cuda"
        host = got.cpu().numpy()
        for i in range(n):
            ref = RR.full_render(stt["cells"][i], tuple(stt["goal_pos"][i]), tuple(stt["agent_pos"][i]),
                                 int(stt["agent_dir"][i]), ts, True)
            assert (host[i] == ref).all(), (i, ts)
        walls, goal, agent = env.snapshot()
        assert (walls.cpu().numpy().view(np.uint32) == stt["walls"]).all()
        assert (goal.cpu().numpy() == stt["goal_pos"]).all()
        assert (agent.cpu().numpy()[:, :2] == stt["agent_pos"]).all()
        assert (agent.cpu().numpy()[:, 2] == stt["agent_dir"]).all() and (agent.cpu().numpy()[:, 3] == 0).all()
        assert torch.equal(nat.render_frames(walls, goal, agent, size, ts, True), got)
        return got

    check(8)
    for t in range(1, 13):
        env.step(torch.from_numpy(rs.randint(0, 3, size=n).astype(np.int64)).to(device), autoreset=True)
        if t in (3, 7, 12):
            full = check(8)
    # index= subsets, highlight off, out=
    idx = torch.tensor([5, 0, 69, 5], dtype=torch.int64, device=device)
    assert torch.equal(env.render_frames(8, index=idx), full[idx])
    stt = env.get_state()
    plain = env.render_frames(5, highlight=False, index=idx[:2]).cpu().numpy()
    for k, i in enumerate([5, 0]):
        assert (plain[k] == RR.full_render(stt["cells"][i], tuple(stt["goal_pos"][i]), tuple(stt["agent_pos"][i]),
                                           int(stt["agent_dir"][i]), 5, False)).all()
    out = torch.zeros((4, size * 8, size * 8, 3), dtype=torch.uint8, device=device)
    assert env.render_frames(8, index=idx, out=out).data_ptr() == out.data_ptr() and torch.equal(out, full[idx])
    with pytest.raises(nat.MerlinNativeError):
        env.render_frames(8, index=idx, out=torch.zeros((4, size * 8, size * 8, 6), dtype=torch.uint8,
                                                        device=device)[..., ::2])
    with pytest.raises(nat.MerlinNativeError):
        env.render_frames(8, out=out)  # 4 frames' room for 70
    with pytest.raises(nat.MerlinNativeError):
        env.render_frames(33)
    env.errors()
    # an env id past the envs: flagged, not read
    env.render_frames(8, index=torch.tensor([70], dtype=torch.int64, device=device))
    assert env.errors(raise_on_error=False)[0] == nat.DEVERR_BAD_FRAME
    env.close()


def test_single_env_render(device):
    from merlin import MerlinEnv, MerlinVecEnv

    S = 9
    env = MerlinEnv(difficulty="mediumhard", size=S, device=device, render_mode="rgb_array")
    vec = MerlinVecEnv(1, difficulty="mediumhard", size=S, device=device, seeds=[31])
    env.reset(seed=31)
    vec.reset()
    for a in [None, 2, 0, 2, 1, 2]:
        if a is not None:
            env.step(a)
            vec.step(torch.tensor([a], device=device), autoreset=False)
        img = env.render()
        assert isinstance(img, np.ndarray) and img.shape == (S * 32, S * 32, 3) and img.dtype == np.uint8
        assert (img == vec.render_frames()[0].cpu().numpy()).all()
        st = env.vec.get_state()
        assert (img == RR.full_render(st["cells"][0], tuple(st["goal_pos"][0]), tuple(st["agent_pos"][0]),
                                      int(st["agent_dir"][0]), 32, True)).all()
    small = env.get_frame(highlight=False, tile_size=6)
    assert small.shape == (S * 6, S * 6, 3)
    assert (small == RR.full_render(st["cells"][0], tuple(st["goal_pos"][0]), tuple(st["agent_pos"][0]),
                                    int(st["agent_dir"][0]), 6, False)).all()
    env.close()
    vec.close()


def test_render_mode_human_is_refused(device):
    from merlin import MerlinEnv

    with pytest.raises(ValueError, match="ppo_visualization"):
        MerlinEnv(size=9, device=device, render_mode="human")
    with pytest.raises(ValueError):
        MerlinEnv(size=9, device=device, render_mode="ansi")
