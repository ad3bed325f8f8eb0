"""GPU: the policy field's two kernels and what is built on them.

k_view_codes   against the C oracle's observations along random rollouts at every grid size of test_gpu_env_sizes'
               matrix (independent of the env kernel), then against the env kernel's own observations, so the two
               nibble packers are held together; invalid poses.
k_policy_paths against the library's host restatement (a forward walk with memoisation) and the tests' own walk
               (tests/policy_field_ref.py), on random, bouncer, shortest-path and all-left action fields; a snake whose
               chain is longer than 1,000 layers.
End to end     evaluate_seeds' rewards and steps equal PolicyField.predicted_episode seed by seed, for scripted
               code-policies, for fresh CNNs, and through the analysis CLI.

n = 130 queries / M = 9 maps: the last block is partial and, for the paths kernel (two maps per wave), the last
wave's second half has no map."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pathing_ref import N, P_FWD, SEED0
from policy_field_ref import (CASES, IDS, SEEDS9, AlwaysLeft, Bouncer, Seeker, bouncer_field, oracle_maps,
                              seeker_field, walk)
from test_policy_field_host import M9, oracle_field, random_field

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = list(range(SEED0, SEED0 + N))
T = 40


def pack(codes49: np.ndarray) -> np.ndarray:
    """uint8[..., 49] tile classes -> int32[..., 8] nibble words, cell (vi, vj) at nibble vj * 7 + vi."""
    nib = np.zeros(codes49.shape[:-1] + (64,), dtype=np.uint32)
    nib[..., :49] = codes49
    w = (nib.reshape(*codes49.shape[:-1], 8, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(-1, dtype=np.uint64)
    return w.astype(np.uint32).view(np.int32)


def dev(a, device, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:  # wall rows: the same bits as int32 (row 31's border bit is the sign)
        a = a.view(np.int32)
    t = torch.from_numpy(a)
    return (t if dtype is None else t.to(dtype)).to(device)


def make_env(device, diff, size, n=N, **kw):
    from merlin import MerlinVecEnv

    return MerlinVecEnv(n, difficulty=diff, size=size, seeds=list(range(SEED0, SEED0 + n)), device=device, **kw)


# -- view_codes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_view_codes_vs_oracle(oracle, device, diff, size):
    """Every observation of a random rollout up to each env's first done, recomputed from (map, pose) alone."""
    from merlin import _native as nat

    acts = np.random.RandomState(3 * size + len(diff)).choice([0, 1, 2], size=(T, N), p=P_FWD).astype(np.int64)
    codes, _, term, trunc, agent = oracle.batch_rollout(np.array(SEEDS, dtype=np.uint64), acts, size=size,
                                                        difficulty=diff)
    _, walls, goal, start = oracle_maps(oracle, diff, size, SEEDS)
    assert (agent[0, :, :3] == start[:, :3]).all()
    done = np.maximum(term, trunc).astype(bool)
    first = np.where(done.any(0), done.argmax(0), T)          # codes[t] belongs to the seeded map for t <= first
    t, i = np.nonzero(np.arange(T + 1)[:, None] <= first[None, :])
    assert len(t) >= 10 * N and (agent[t, i, :2] != start[i, :2]).any(1).sum() >= N  # the agents did move
    pose = agent[t, i].copy()
    pose[:, 3] = 0
    got = nat.view_codes(dev(walls, device, torch.int32), dev(goal, device), dev(pose, device), size,
                         map_index=dev(i.astype(np.int32), device))
    assert got.dtype == torch.int32 and got.shape == (len(t), 8)
    bad = np.flatnonzero((got.cpu().numpy() != pack(codes[t, i])).any(1))
    assert len(bad) == 0, (bad[:5], t[bad[:5]], i[bad[:5]])
    assert nat.tower_errors(device) == 0


@pytest.mark.parametrize("diff,size,n", [("mediumhard", 16, N), ("hard", 31, 129), ("easy", 5, 1), ("hardest", 32, N)])
def test_view_codes_vs_env(device, diff, size, n):
    """The env's own observation after a reset and after 40 random steps with auto-reset, from its snapshot; the
    output is a slice of a guarded buffer."""
    from merlin import _native as nat

    env = make_env(device, diff, size, n=n)
    obs = env.reset().clone()
    acts = dev(np.random.RandomState(size).choice([0, 1, 2], size=(T, n), p=P_FWD).astype(np.int64), device)
    for t in range(T + 1):
        walls, goal, agent = env.snapshot()
        guard = torch.full((n + 4, 8), 0x5A5A5A5A, dtype=torch.int32, device=device)
        out = nat.view_codes(walls, goal, agent, size, out=guard[2:n + 2])
        assert out.data_ptr() == guard[2:].data_ptr()
        assert torch.equal(out, obs), t
        assert (guard[:2] == 0x5A5A5A5A).all() and (guard[n + 2:] == 0x5A5A5A5A).all()
        if t in (0, T):  # the narrow store path: an output 4 bytes off
            flat = torch.full((n * 8 + 9,), 0x5A5A5A5A, dtype=torch.int32, device=device)
            nat.view_codes(walls, goal, agent, size, out=flat[1:n * 8 + 1])
            assert torch.equal(flat[1:n * 8 + 1].view(n, 8), obs) and (flat[0] == 0x5A5A5A5A) and \
                (flat[n * 8 + 1:] == 0x5A5A5A5A).all()
        if t < T:
            obs = env.step(acts[t])[0].clone()
    assert env.errors() == (0, 0) and nat.tower_errors(device) == 0
    env.close()


def test_view_codes_invalid_poses(oracle, device):
    from merlin import _native as nat

    size = 11
    cells, walls, goal, start = oracle_maps(oracle, "mediumhard", size, SEEDS[:4])
    wy, wx = np.argwhere(cells[1, 1:-1, 1:-1] == 1)[0] + 1  # an inner wall of map 1
    pose = np.array([start[0], (wx, wy, 0, 0), start[1], (-1, 3, 1, 0), (size, 3, 1, 0), start[2],
                     (start[3, 0], start[3, 1], 4, 0), start[3]], dtype=np.int32)
    pose[:, 3] = 0
    index = np.array([0, 1, 1, 2, 2, 2, 3, 3], dtype=np.int32)
    w, g = dev(walls, device, torch.int32), dev(goal, device)
    nat.tower_errors(device, raise_on_error=False)
    got = nat.view_codes(w, g, dev(pose, device), size, map_index=dev(index, device))
    flags = nat.tower_errors(device, raise_on_error=False)
    assert flags & nat.DEVERR_BAD_FRAME and not flags & nat.DEVERR_BAD_TILE
    bad = [1, 3, 4, 6]
    good = [0, 2, 5, 7]
    assert (got[bad] == 0).all()
    alone = nat.view_codes(w, g, dev(pose[good], device), size, map_index=dev(index[good], device))
    assert torch.equal(got[good], alone) and ((alone[:, 5] >> 20) & 0xF == 4).all()  # the agent tile at nibble 45
    assert nat.tower_errors(device) == 0
    # without a goal, and with one outside the grid: the same view with the goal tile (class 3) read as empty (1)
    for no_goal in (None, torch.full_like(g, -1), torch.full_like(g, size)):
        ng = nat.view_codes(w, no_goal, dev(pose[good], device), size, map_index=dev(index[good], device))
        nib_a = (alone.unsqueeze(-1) >> (4 * torch.arange(8, device=device, dtype=torch.int32))) & 0xF
        nib_n = (ng.unsqueeze(-1) >> (4 * torch.arange(8, device=device, dtype=torch.int32))) & 0xF
        assert torch.equal(torch.where(nib_a == 3, torch.ones_like(nib_a), nib_a), nib_n)
    with pytest.raises(nat.MerlinNativeError):
        nat.view_codes(w, g, dev(pose, device), size, map_index=dev(index + 1, device))
    with pytest.raises(nat.MerlinNativeError):
        nat.view_codes(w, g, dev(pose[:1], device), size, map_index=dev(index[:1], device))
        nat.view_codes(w, g, dev(pose[1:2], device), size, map_index=dev(index[1:2], device))
        nat.tower_errors(device)


# -- policy_paths ----------------------------------------------------------------------------------------------------
def run_paths(nat, device, walls, goal, action, size):
    """The kernel into an output that starts 2 bytes off any wider alignment, guards on both sides."""
    m = walls.shape[0]
    k = m * 4 * size * size
    buf = torch.full((k + 16,), 321, dtype=torch.int16, device=device)
    out = nat.policy_paths(dev(walls, device, torch.int32), dev(goal, device), dev(action, device), size,
                           out=buf[1:k + 1])
    assert out.data_ptr() % 4 == 2 and out.shape == (m, 4, size, size)
    assert int(buf[0]) == 321 and (buf[k + 1:] == 321).all()
    return out.cpu().numpy()


@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_policy_paths_vs_host(oracle, device, diff, size):
    from merlin import _native as nat

    cells, walls, goal, _ = oracle_maps(oracle, diff, size, SEEDS9)
    opt, dist = oracle_field(nat, walls, goal, size)
    fields = {"random": random_field(size, 11 * size + len(diff)),
              "bouncer": np.stack([bouncer_field(c) for c in cells]),
              "seeker": np.stack([seeker_field(c, g) for c, g in zip(cells, goal)]),
              "oracle": opt,
              "left": np.zeros((M9, 4, size, size), dtype=np.int8)}
    for name, a in fields.items():
        got = run_paths(nat, device, walls, goal, a, size)
        want = nat.policy_paths_host(walls, goal, a, size)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, bad[:5])
        one = run_paths(nat, device, walls[-1:], goal[-1:], a[-1:], size)  # M = 1: a block of one half wave
        assert (one == want[-1:]).all(), name
    assert (run_paths(nat, device, walls, goal, opt, size) == dist).all()
    assert (run_paths(nat, device, walls, goal, fields["left"], size) == -1).all()
    r = run_paths(nat, device, walls, goal, fields["random"], size)
    assert (r == walk(cells, goal, fields["random"])).all()
    if size <= 17:
        assert (run_paths(nat, device, walls, goal, fields["bouncer"], size) == walk(cells, goal, fields["bouncer"])).all()


def snake(size=32):
    """A path that turns in every cell -- strips two cells wide, walked in zigzag, down one strip and up the next --
    and the policy that follows it: about two actions per cell.  Every cell off the path is a wall, the path's last
    cell is the goal.  -> (cells, goal, action int8[4, S, S], the start pose)."""
    vec = ((1, 0), (0, 1), (-1, 0), (0, -1))
    path = []
    for s in range((size - 2) // 2):
        cols = [1 + 2 * s, 2 + 2 * s]
        rows = range(2, size - 1) if s % 2 == 0 else range(size - 2, 1, -1)
        c = 0
        for y in rows:  # the row's two cells, starting in the column the last row ended in
            path += [(cols[c], y), (cols[1 - c], y)]
            c = 1 - c
    assert len(set(path)) == len(path) and all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(path, path[1:]))
    cells = np.ones((size, size), dtype=np.uint8)
    for x, y in path:
        cells[y, x] = 0
    action = np.zeros((4, size, size), dtype=np.int8)  # everything off the chain turns left for ever
    d = 3
    start = (path[0][0], path[0][1], d, 0)
    for (x, y), (nx, ny) in zip(path, path[1:]):
        nd = vec.index((nx - x, ny - y))
        while d != nd:
            turn = 0 if (d + 3) & 3 == nd else 1
            action[d, y, x] = turn
            d = (d + 3) & 3 if turn == 0 else (d + 1) & 3
        action[d, y, x] = 2
    return cells, np.array(path[-1], dtype=np.int32), action, np.array(start, dtype=np.int32)


def test_policy_paths_snake(device):
    """A chain of more than 1,000 layers at size 32: the layer loop runs far past any shortest path's length."""
    from merlin import _native as nat

    cells, goal, action, start = snake()
    want = walk(cells, goal, action)
    x, y, d, _ = start
    assert want.max() >= want[d, y, x] > 1000  # (a pose that turns into the start pose is one layer further)
    assert set(want[want > 0].tolist()) == set(range(1, int(want.max()) + 1))  # every layer holds a pose
    walls = ((cells == 1).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    # three maps: the snake, an open map beside it in the same wave, the snake again in a wave's first half alone
    blank = np.zeros_like(cells)
    blank[0, :] = blank[-1, :] = blank[:, 0] = blank[:, -1] = 1
    bw = ((blank == 1).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    W = np.stack([walls, bw, walls])
    G = np.stack([goal, goal, goal])
    A = np.stack([action, np.full_like(action, 2), action])
    got = run_paths(nat, device, W, G, A, 32)
    assert (got[0] == want).all() and (got[2] == want).all()
    assert (got == nat.policy_paths_host(W, G, A, 32)).all()
    assert (got[1] == walk(blank, goal, A[1])).all()


def test_captured_into_a_graph(oracle, device):
    """Both kernels on a capturing side stream: replayed after the inputs were overwritten, the results equal eager
    calls on the new inputs."""
    from merlin import _native as nat

    size = 17
    _, walls, goal, start = oracle_maps(oracle, "hard", size, SEEDS)
    _, walls2, goal2, start2 = oracle_maps(oracle, "mediumhard", size, SEEDS)
    start, start2 = start.copy(), start2.copy()
    start[:, 3] = start2[:, 3] = 0
    rs = np.random.RandomState(1)
    act, act2 = (rs.randint(0, 3, size=(N, 4, size, size)).astype(np.int8) for _ in range(2))
    w, g, a, p = dev(walls, device, torch.int32), dev(goal, device), dev(act, device), dev(start, device)
    codes = torch.zeros((N, 8), dtype=torch.int32, device=device)
    steps = torch.zeros((N, 4, size, size), dtype=torch.int16, device=device)
    nat.view_codes(w, g, p, size, out=codes)  # warm-up: the device's error word exists
    nat.policy_paths(w, g, a, size, out=steps)
    first = (codes.clone(), steps.clone())
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            nat.view_codes(w, g, p, size, out=codes)
            nat.policy_paths(w, g, a, size, out=steps)
    w.copy_(dev(walls2, device, torch.int32))
    g.copy_(dev(goal2, device))
    a.copy_(dev(act2, device))
    p.copy_(dev(start2, device))
    codes.zero_()
    steps.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(codes, nat.view_codes(w, g, p, size)) and not torch.equal(codes, first[0])
    assert torch.equal(steps, nat.policy_paths(w, g, a, size)) and not torch.equal(steps, first[1])
    assert (steps.cpu().numpy() == nat.policy_paths_host(walls2, goal2, act2, size)).all()
    del graph


# -- end to end ------------------------------------------------------------------------------------------------------
E2E_CASES = [("medium", 8), ("mediumhard", 16), ("hard", 17)]


def episodes_match(ac, diff, size, device):
    from merlin.evaluation import evaluate_seeds
    from merlin.policy_field import policy_field_for_seeds

    rew, steps = evaluate_seeds(ac, SEEDS, difficulty=diff, size=size, device=device)
    field, agent, ms = policy_field_for_seeds(ac, SEEDS, difficulty=diff, size=size, device=device)
    assert ms == 4 * size * size
    pr, ps = field.predicted_episode(agent, ms)
    rew = np.asarray(rew, dtype=np.float64).astype(np.float32)
    return field, agent, (rew == pr.cpu().numpy()) & (np.asarray(steps) == ps.cpu().numpy()), rew


@pytest.mark.parametrize("diff,size", E2E_CASES)
def test_scripted_policies_end_to_end(oracle, device, diff, size):
    """evaluate_seeds equals the field's prediction for every seed and scripted policy.  Not vacuous -- on the CPU,
    from the oracle's maps and walk alone, succeeded / failed of 130: Bouncer 71 / 59 on medium 8, 27 / 103 on
    mediumhard 16, 12 / 118 on hard 17; Seeker 39 / 91, 11 / 119 and 1 / 129."""
    cells, _, goal, start = oracle_maps(oracle, diff, size, SEEDS)
    ms = 4 * size * size
    tally = {}
    for policy, restated in ((Bouncer(), np.stack([bouncer_field(c) for c in cells])),
                             (Seeker(), np.stack([seeker_field(c, g) for c, g in zip(cells, goal)])),
                             (AlwaysLeft(), np.zeros((N, 4, size, size), dtype=np.int8))):
        want = walk(cells, goal, restated)[np.arange(N), start[:, 2], start[:, 1], start[:, 0]]
        won = (want >= 1) & (want <= ms)
        tally[type(policy).__name__] = (int(won.sum()), int((~won).sum()))
        field, agent, same, rew = episodes_match(policy, diff, size, device)
        assert (agent.cpu().numpy()[:, :3] == start[:, :3]).all()
        assert same.all(), (type(policy).__name__, np.flatnonzero(~same)[:5])
        assert ((rew > 0) == won).all()
        # the policy read off the view codes is the one written from the cells
        free = field.free.cpu().numpy()
        assert (field.action.cpu().numpy()[free] == restated[free]).all()
        assert (field.steps.cpu().numpy() == walk(cells, goal, np.where(free, restated, -1))).all()
    assert tally["AlwaysLeft"] == (0, N)
    expected = {("medium", 8): ((71, 59), (39, 91)), ("mediumhard", 16): ((27, 103), (11, 119)),
                ("hard", 17): ((12, 118), (1, 129))}[(diff, size)]
    assert (tally["Bouncer"], tally["Seeker"]) == expected
    if (diff, size) == ("medium", 8):
        assert min(tally["Bouncer"]) >= 10 and min(tally["Seeker"]) >= 10


CNN_TORCH_SEEDS = (0, 1, 2)


def fresh_cnn(torch_seed, device):
    """A fresh CNNActorCritic whose actor head's last layer is scaled by 100: a decisive argmax."""
    from merlin.actor_critic import CNNActorCritic

    torch.manual_seed(torch_seed)
    ac = CNNActorCritic((56, 56, 3), 3)
    with torch.no_grad():
        ac.actor[2].weight *= 100.0
        ac.actor[2].bias *= 100.0
    return ac.to(device)


@pytest.mark.parametrize("diff,size", E2E_CASES[:2])
def test_cnn_end_to_end(device, diff, size):
    """The same equality for fresh CNNs.  The field's forward runs all free poses in one batch and evaluate_seeds 130
    frames a step, so a seed may be left out only if its predicted trajectory visits a pose whose top-2 logit margin
    is below 1e-5, and at most 10 % of the seeds are.  (On the CPU, with these torch seeds, ac.act on the oracle's
    frames meets no such pose on any trajectory.)"""
    for torch_seed in CNN_TORCH_SEEDS:
        ac = fresh_cnn(torch_seed, device)
        field, agent, same, _ = episodes_match(ac, diff, size, device)
        if same.all():
            continue
        with torch.no_grad():
            logits, _ = ac._forward_codes(field.codes)
        top = logits.topk(2, dim=-1).values
        margin = (top[:, 0] - top[:, 1]).cpu().numpy()
        n = field.codes.shape[0]
        row = np.full((N, 4, size, size), -1, dtype=np.int64)
        ag, mi = field.agent.cpu().numpy(), field.map_index.cpu().numpy()
        row[mi, ag[:, 2], ag[:, 1], ag[:, 0]] = np.arange(n)
        action = field.action.cpu().numpy()
        cells = ~field.free.cpu().numpy()[:, 0]
        goal = field.goal.cpu().numpy()
        vec = ((1, 0), (0, 1), (-1, 0), (0, -1))
        excused = []
        for i in np.flatnonzero(~same):
            x, y, d = (int(v) for v in agent[i, :3].cpu())
            seen, close = set(), False
            while (x, y, d) not in seen:  # the predicted trajectory: to termination, a dead end or round its cycle
                seen.add((x, y, d))
                close |= margin[row[i, d, y, x]] < 1e-5
                a = action[i, d, y, x]
                if a == 0:
                    d = (d + 3) & 3
                elif a == 1:
                    d = (d + 1) & 3
                else:
                    fx, fy = x + vec[d][0], y + vec[d][1]
                    if cells[i, fy, fx] or (fx, fy) == tuple(goal[i]):
                        break
                    x, y = fx, fy
            assert close, (torch_seed, int(i))
            excused.append(int(i))
        assert len(excused) <= N // 10, (torch_seed, excused)


YAML = """
global:
  max_steps: 48
difficulties:
  easy:
    env_id: MERLIN-Easy-v0
    params: {render_mode: rgb_array, size: 8}
  medium:
    env_id: MERLIN-Medium-v0
    params: {render_mode: rgb_array, size: 8}
"""


def test_cli(device, tmp_path):
    from merlin.actor_critic import CNNActorCritic
    from merlin.checkpoints import load_policy
    from merlin.evaluation import evaluate_seeds

    torch.manual_seed(5)
    torch.save(CNNActorCritic((56, 56, 3), 3).state_dict(), tmp_path / "ppo_model_1k.pth")
    (tmp_path / "scenario.yaml").write_text(YAML)
    out_dir = tmp_path / "field"
    r = subprocess.run([sys.executable, os.path.join(REPO, "ppo-2dgrid_amd", "analyze_policy_field.py"), "--config",
                        str(tmp_path / "scenario.yaml"), "--model_path", str(tmp_path / "ppo_model_1k.pth"),
                        "--difficulties", "easy", "medium", "--num_tasks", "8", "--base_seed", "4000", "--size", "8",
                        "--out_dir", str(out_dir), "--no_plots"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out_dir)) == ["policy_field.json"]
    res = json.loads((out_dir / "policy_field.json").read_text())
    assert res["size"] == 8 and res["max_steps"] == 48 and res["difficulties"] == ["easy", "medium"]
    ac = load_policy(str(tmp_path / "ppo_model_1k.pth"), device)
    for d in ("easy", "medium"):
        p = res["per_difficulty"][d]
        assert {"solved_rate", "trapped_rate", "timeout_rate", "spl", "excess_steps", "optimal_action_rate",
                "value_rmse", "n_solvable"} <= set(p["field"])
        f = p["field"]
        if f["n_solvable"]:
            assert abs(f["solved_rate"] + f["trapped_rate"] + f["timeout_rate"] - 1.0) < 1e-12
        rew, steps = evaluate_seeds(ac, range(4000, 4008), difficulty=d, size=8, device=device, max_steps=48)
        assert p["start"]["seeds"] == list(range(4000, 4008))
        assert p["start"]["steps"] == steps
        assert p["start"]["rewards"] == np.asarray(rew, dtype=np.float64).astype(np.float32).astype(np.float64).tolist()
