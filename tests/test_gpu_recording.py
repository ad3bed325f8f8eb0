"""GPU: recorded episodes (merlin.recording) and the playback CLI (ppo_visualization.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import minigrid_literal as ML
import render_ref as RR

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, MAX_STEPS, SEEDS, DIFF = 9, 24, list(range(500, 508)), "mediumhard"


@pytest.fixture(scope="module")
def policy(device):
    from merlin.actor_critic import CNNActorCritic

    torch.manual_seed(3)
    return CNNActorCritic((56, 56, 3), 3).to(device).eval()


@pytest.fixture(scope="module")
def rec(policy, device):
    from merlin.recording import record_episodes

    return record_episodes(policy, SEEDS, difficulty=DIFF, size=SIZE, device=device, max_steps=MAX_STEPS)


def test_recording_matches_the_evaluator(rec, policy, device):
    from merlin.evaluation import evaluate_seeds

    rew, steps = evaluate_seeds(policy, SEEDS, difficulty=DIFF, size=SIZE, device=device, max_steps=MAX_STEPS)
    assert rec.returns.tolist() == rew and rec.lengths.tolist() == steps
    T = int(rec.actions.shape[0])
    assert T == max(steps) and rec.agent.shape == (T + 1, len(SEEDS), 4) and rec.rewards.shape == (T, len(SEEDS))
    for i, n in enumerate(steps):
        # frozen at the first done: the state repeats, the rewards stop
        assert (rec.agent[n:, i] == rec.agent[n, i]).all() and (rec.rewards[n:, i] == 0).all()
        assert len(rec.frames(i, tile_size=5)) == n + 1


def test_frames_follow_a_literal_replay(rec):
    """Frame 0 is the reset state; frame t the state after the first t recorded actions, replayed by the literal
    Python env."""
    ts = 8
    for i, seed in enumerate(SEEDS):
        lit = ML.LiteralEnv(size=SIZE, difficulty=DIFF, max_steps=MAX_STEPS)
        lit.reset(seed=seed)
        frames = rec.frames(i, tile_size=ts)
        n = int(rec.lengths[i])
        assert frames.shape == (n + 1, SIZE * ts, SIZE * ts, 3)
        for t in range(n + 1):
            if t > 0:
                lit.step(int(rec.actions[t - 1, i]))
            ref = RR.full_render(lit.cells(), tuple(lit.goal_pos), tuple(lit.agent_pos), lit.agent_dir, ts, True)
            assert (frames[t] == ref).all(), (seed, t)


def test_chunked_rendering_equals_unchunked(rec, monkeypatch):
    i = int(rec.lengths.argmax())
    whole = rec.frames(i, tile_size=8)
    fb = (SIZE * 8) ** 2 * 3
    monkeypatch.setattr(rec, "chunk_bytes", 3 * fb + 100)  # three frames per launch
    chunks = list(rec.iter_frames(i, tile_size=8))
    assert len(chunks) == -(-len(whole) // 3) and all(c.shape[0] <= 3 for c in chunks)
    assert (rec.frames(i, tile_size=8) == whole).all()
    assert (rec.frames(i, tile_size=8, start=2, stop=7) == whole[2:7]).all()
    monkeypatch.setattr(rec, "chunk_bytes", 1)  # never less than one frame per launch
    assert (rec.frames(i, tile_size=8, stop=4) == whole[:4]).all()


def test_npz_round_trip(rec, tmp_path, device):
    from merlin.recording import Recording

    path = rec.save_npz(str(tmp_path / "rec.npz"))
    back = Recording.load_npz(path, device=device)
    assert back.seeds == rec.seeds and back.difficulty == rec.difficulty
    assert (back.size, back.max_steps) == (rec.size, rec.max_steps)
    for name in ("walls", "goal", "agent", "actions", "rewards", "lengths", "returns"):
        assert torch.equal(getattr(back, name), getattr(rec, name)), name
    assert (back.frames(1, tile_size=5) == rec.frames(1, tile_size=5)).all()
    assert os.path.getsize(path) < 64 * 1024  # the compact recording, not the pixels


def test_gif_and_contact_sheet(rec, tmp_path):
    from PIL import Image

    i, ts, fps = 0, 8, 20
    frames = rec.frames(i, tile_size=ts)
    path = rec.save_gif(str(tmp_path / "ep.gif"), i, fps=fps, tile_size=ts)
    with Image.open(path) as im:
        assert im.size == (SIZE * ts, SIZE * ts)
        # GIF writers fold a frame identical to its predecessor (a step into a wall) into that frame's duration:
        # the file holds the episode's distinct consecutive frames, and its durations add up to all of them
        distinct = 1 + sum(bool((frames[t] != frames[t - 1]).any()) for t in range(1, len(frames)))
        assert im.n_frames == distinct
        total = 0
        for k in range(im.n_frames):
            im.seek(k)
            total += im.info["duration"]
        assert total == len(frames) * (1000 // fps)
        im.seek(0)
        assert (np.asarray(im.convert("RGB")) == frames[0]).all()
    sheet = rec.contact_sheet(indices=[0, 3, 5], step="last", tile_size=5, cols=2)
    side = SIZE * 5
    assert sheet.shape == (2 * side, 2 * side, 3)
    for p, e in enumerate([0, 3, 5]):
        r, c = divmod(p, 2)
        assert (sheet[r * side:(r + 1) * side, c * side:(c + 1) * side] == rec.frames(e, tile_size=5)[-1]).all()
    assert (sheet[side:, side:] == 0).all()
    assert (rec.contact_sheet(indices=[2], step=0, tile_size=5) == rec.frames(2, tile_size=5)[0]).all()


def _run_cli(tmp_path, model, extra):
    script = os.path.join(REPO, "ppo-2dgrid_amd", "ppo_visualization.py")
    out = tmp_path / "renders"
    r = subprocess.run([sys.executable, script, "--episodes", "2", "--difficulty", "easy", "--tile_size", "8",
                        "--max_steps", "24", "--model_path", str(model), "--out_dir", str(out)] + extra,
                       cwd=tmp_path, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return out, r.stdout


def _averages(stdout):
    return ([float(x) for x in re.findall(r"Average Reward: (-?\d+\.\d{3})", stdout)],
            [float(x) for x in re.findall(r"Average Steps : (\d+\.\d)", stdout)])


def test_cli_writes_gifs_and_summary(policy, tmp_path):
    from PIL import Image

    model = tmp_path / "fresh.pth"
    torch.save(policy.state_dict(), model)
    out, stdout = _run_cli(tmp_path, model, [])
    names = sorted(os.listdir(out))
    assert names == ["episode_1_seed_124.gif", "episode_2_seed_125.gif", "summary.png"], names
    assert len(re.findall(r"Episode +\d+ \| Reward: -?\d+\.\d{3} \| Steps: \d+", stdout)) == 2
    rew, steps = _averages(stdout)
    assert len(rew) == 1 and len(steps) == 1 and 1 <= steps[0] <= 24
    with Image.open(out / "episode_1_seed_124.gif") as im:
        assert im.size == (16 * 8, 16 * 8)
    with Image.open(out / "summary.png") as im:
        assert im.size == (2 * 16 * 8, 16 * 8)


def test_cli_adaptation_writes_pre_and_post(policy, tmp_path):
    model = tmp_path / "fresh.pth"
    torch.save(policy.state_dict(), model)
    out, stdout = _run_cli(tmp_path, model, ["--adapt_steps", "1", "--k_support", "32"])
    names = set(os.listdir(out))
    want = {f"episode_{ep}_seed_{123 + ep}_{w}.gif" for ep in (1, 2) for w in ("pre", "post")}
    assert want | {"summary_pre.png", "summary_post.png"} == names, names
    rew, steps = _averages(stdout)
    assert len(rew) == 2 and len(steps) == 2
