"""GPU: the shortest-path kernel (k_shortest_paths) against a forward breadth-first search written from the step rule
(tests/pathing_ref.py) and against the library's host solver, at every grid size of test_gpu_env_sizes' matrix; then
end to end through the real step kernel (a greedy walk down the distance field terminates at exactly dist with exactly
the optimal reward), as a lower bound on arbitrary behaviour, stateless with a map index, captured into a graph, and
through merlin.pathing and the two analysis CLIs.

n = 130 envs: 65 env pairs (a kernel wave holds two envs), so the last 8-env block is partial; n = 129 leaves half of
the last wave without an env."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pathing_ref import CASES, IDS, N, P_FWD, SEED0, bfs, bfs_state, oracle_maps

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = list(range(SEED0, SEED0 + N))


def make_env(device, diff, size, n=N, **kw):
    from merlin import MerlinVecEnv

    return MerlinVecEnv(n, difficulty=diff, size=size, seeds=list(range(SEED0, SEED0 + n)), device=device, **kw)


def host_of(nat, env, field=True):
    walls, goal, agent = (t.cpu().numpy() for t in env.snapshot())
    return nat.shortest_paths_host(walls, goal, agent, env.size, field=field)


@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_optimal_steps_after_reset(device, diff, size):
    from merlin import _native as nat

    env = make_env(device, diff, size)
    env.reset()
    st = env.get_state()
    dist = env.optimal_steps()
    assert dist.dtype == torch.int32 and dist.shape == (N,)
    dist = dist.cpu().numpy()
    idx = range(32 if size >= 31 else N)
    want = bfs_state(st, idx)
    assert (dist[:len(idx)] == want).all(), np.flatnonzero(dist[:len(idx)] != want)
    d2, field = env.distance_field()
    hd, hf = host_of(nat, env)
    assert field.dtype == torch.int16 and field.shape == (N, 4, size, size)
    assert (dist == hd).all() and (d2.cpu().numpy() == hd).all()
    bad = np.argwhere(field.cpu().numpy() != hf)
    assert len(bad) == 0, bad[:5]
    assert env.errors() == (0, 0)
    env.close()


@pytest.mark.parametrize("diff,size", [("mediumhard", 16), ("hard", 17)])
def test_half_empty_last_wave(device, diff, size):
    """n = 129: the last wave's second half has no env; n = 1: a block of one half wave."""
    from merlin import _native as nat

    for n in (129, 1):
        env = make_env(device, diff, size, n=n)
        env.reset()
        guard = torch.full((n + 64,), 12345, dtype=torch.int32, device=device)
        dist = env.optimal_steps(out=guard[:n])
        fbuf = torch.full((n * 4 * size * size + 1,), 321, dtype=torch.int16, device=device)
        walls, goal, agent = env.snapshot()
        sd, sf = nat.shortest_paths(walls, goal, agent, size, field=True)
        hd, hf = host_of(nat, env)
        assert (dist.cpu().numpy() == hd).all() and (guard[n:] == 12345).all()
        assert (sd.cpu().numpy() == hd).all() and (sf.cpu().numpy() == hf).all()
        # the env's own field into a buffer that starts 2 bytes off any wider alignment
        out = fbuf[1:].view(n, 4, size, size)
        assert env.distance_field(out=out)[1] is out
        assert (out.cpu().numpy() == hf).all() and int(fbuf[0]) == 321
        env.close()


def test_conditions_occur(oracle, device):
    """On-goal starts, an unreachable goal and the horizon split: present in the CPU oracle's maps (so the test cannot
    pass by missing them), and answered by the kernel."""
    from merlin.pathing import optimal_reward

    # easy 6: 10 envs start on the goal; the goal cell is an ordinary cell for them
    _, _, goal, agent = oracle_maps(oracle, "easy", 6, SEEDS)
    on_goal = (agent[:, :2] == goal).all(1)
    assert on_goal.sum() == 10
    env = make_env(device, "easy", 6)
    env.reset()
    dist = env.optimal_steps().cpu().numpy()
    assert set(dist[on_goal]) <= {4, 5} and (dist != 0).all()
    env.close()
    # easy 5: the goal is the border's corner (0, 0), which no cell faces
    _, _, goal, _ = oracle_maps(oracle, "easy", 5, SEEDS)
    assert (goal == 0).all()
    env = make_env(device, "easy", 5)
    env.reset()
    dist = env.optimal_steps()
    assert (dist == -1).all() and (optimal_reward(dist, env.max_steps) == 0).all()
    env.close()
    # hard 17 with episodes of 20: 38 beyond the horizon, 92 inside, 7 exactly on it
    cells, _, goal, agent = oracle_maps(oracle, "hard", 17, SEEDS)
    want = np.array([bfs(cells[i], agent[i, :2], agent[i, 2], goal[i]) for i in range(N)])
    assert ((want > 20).sum(), ((want >= 1) & (want <= 20)).sum(), (want == 20).sum()) == (38, 92, 7)
    env = make_env(device, "hard", 17, max_steps=20)
    env.reset()
    dist = env.optimal_steps()
    assert (dist.cpu().numpy() == want).all()
    r = optimal_reward(dist, env.max_steps).cpu().numpy()
    assert r.dtype == np.float32
    assert (r[want > 20] == 0).all() and (r[want == 20] == np.float32(0.1)).all() and (r[want <= 20] > 0).all()
    env.close()


@pytest.mark.parametrize("diff,size", [("mediumhard", 15), ("hardest", 17)])
def test_mid_episode_poses(device, diff, size):
    from merlin import _native as nat

    env = make_env(device, diff, size)
    env.reset()
    acts = torch.from_numpy(np.random.RandomState(size).choice([0, 1, 2], size=(40, N), p=P_FWD)).to(device)
    done = torch.zeros(N, dtype=torch.bool, device=device)
    for t in range(40):
        _, _, term, trunc, _ = env.step(acts[t], autoreset=False)
        done |= term | trunc
    running = np.flatnonzero(~done.cpu().numpy())
    assert len(running) >= N // 4
    st = env.get_state()
    moved = (st["step_count"] == 40)[running]
    assert moved.all()
    dist = env.optimal_steps()
    assert (dist.cpu().numpy()[running] == bfs_state(st, running)).all()
    walls, goal, agent = env.snapshot()
    assert torch.equal(nat.shortest_paths(walls, goal, agent, size), dist)
    env.close()


@pytest.mark.parametrize("diff,size,max_steps,n", [("mediumhard", 16, None, N), ("hard", 17, 20, N),
                                                   ("hardest", 32, None, 64)])
def test_greedy_walk(oracle, device, diff, size, max_steps, n):
    """Down the distance field through the real step kernel: every solvable env terminates at exactly step dist with
    exactly the optimal reward (the step's f32 reward, and its f64 episode return rounded to f32), dist falling by one
    per step; the recorded actions replayed by the oracle end the same way."""
    from merlin.pathing import optimal_reward, oracle_actions, path_metrics

    env = make_env(device, diff, size, n=n, max_steps=max_steps)
    env.reset()
    dist0, field = env.distance_field()
    ms = env.max_steps
    solvable = (dist0 >= 1) & (dist0 <= ms)
    assert int(solvable.sum()) >= n // 2
    T = min(ms, int(dist0.max()))
    end = torch.zeros(n, dtype=torch.int64, device=device)       # step of the first done
    ret = torch.zeros(n, dtype=torch.float64, device=device)
    last_rew = torch.zeros(n, dtype=torch.float32, device=device)
    termd = torch.zeros(n, dtype=torch.bool, device=device)
    acts = []
    for t in range(T):
        live = end == 0
        cur = env.optimal_steps()
        on_path = live & (dist0 >= 1)
        assert torch.equal(cur[on_path], dist0[on_path] - t), t
        walls, goal, agent = env.snapshot()
        a = oracle_actions(field, walls, goal, agent)
        assert a.dtype == torch.int64 and a.shape == (n,)
        acts.append(a)
        _, rew, term, trunc, info = env.step(a, autoreset=False)
        fin = live & (term | trunc)
        end = torch.where(fin, torch.full_like(end, t + 1), end)
        ret = torch.where(fin, info["episode_return"], ret)
        last_rew = torch.where(fin, rew, last_rew)
        termd |= live & term
    assert env.errors() == (0, 0)
    env.close()
    opt = optimal_reward(dist0, ms)
    assert torch.equal(termd, solvable)
    assert torch.equal(end[solvable], dist0[solvable].long())
    assert torch.equal(last_rew[solvable], opt[solvable]) and torch.equal(ret.float()[solvable], opt[solvable])
    if max_steps is not None:  # beyond the horizon: truncated at max_steps with nothing
        late = dist0 > ms
        assert int(late.sum()) > 0 and (end[late] == ms).all() and (ret[late] == 0).all() and (opt[late] == 0).all()
    # the oracle's replay of the recorded actions
    A = torch.stack(acts).cpu().numpy()
    _, orew, oterm, otrunc, _ = oracle.batch_rollout(np.arange(SEED0, SEED0 + n, dtype=np.uint64), A, size=size,
                                                     difficulty=diff, max_steps=ms)
    odone = np.maximum(oterm, otrunc)
    has = odone.any(0)
    first = odone.argmax(0)
    d0, sol = dist0.cpu().numpy(), solvable.cpu().numpy()
    assert has[sol].all() and (first[sol] + 1 == d0[sol]).all() and (oterm[first, np.arange(n)][sol] == 1).all()
    assert (orew[first, np.arange(n)][sol] == opt.cpu().numpy()[sol]).all()
    if max_steps is not None:
        late = d0 > ms
        assert (first[late] + 1 == ms).all() and (oterm[first, np.arange(n)][late] == 0).all()
    m = path_metrics(ret.cpu().numpy(), end.cpu().numpy(), d0, ms)
    assert m["n_solvable"] == int(sol.sum()) and m["spl"] == 1.0 and m["regret_mean"] == 0.0
    assert m["success_rate"] == 1.0 and m["reward_ratio"] == 1.0 and m["excess_steps_mean"] == 0.0


def test_lower_bound_on_random_behaviour(device):
    from merlin.pathing import optimal_reward
    from merlin.recording import Recording

    acts = np.random.RandomState(5).randint(0, 3, size=(160, N))
    rec = Recording.from_actions(SEEDS, acts, difficulty="medium", size=8, device=device)
    opt = rec.optimal_steps()
    assert opt.dtype == torch.int64 and opt.shape == (N,) and (opt >= 1).all()
    won = rec.returns > 0
    assert int(won.sum()) >= 10
    assert (rec.lengths[won] >= opt[won]).all()
    assert (rec.returns.float()[won] <= optimal_reward(opt, rec.max_steps)[won]).all()
    assert (rec.lengths[won] == opt[won]).sum() < int(won.sum())  # a bound, not an identity


def test_map_index(device):
    """130 poses spread over 4 maps -- free cells, walls and poses outside the grid -- against the host solver given
    each pose's map."""
    from merlin import _native as nat

    size = 11
    env = make_env(device, "mediumhard", size, n=4)
    env.reset()
    walls, goal, _ = env.snapshot()
    env.close()
    rs = np.random.RandomState(3)
    agent = np.zeros((N, 4), dtype=np.int32)
    agent[:, 0:2] = rs.randint(1, size - 1, size=(N, 2))  # inside the border: free cells and inner walls
    agent[:, 2] = rs.randint(0, 4, size=N)
    agent[100:, 0:2] = rs.randint(-1, size + 1, size=(N - 100, 2))  # the border, and one cell outside the grid
    agent[100:, 2] = rs.randint(-1, 5, size=N - 100)
    index = rs.randint(0, 4, size=N).astype(np.int32)
    assert set(index) == {0, 1, 2, 3}
    hd, hf = nat.shortest_paths_host(walls.cpu().numpy()[index], goal.cpu().numpy()[index], agent, size, field=True)
    assert (hd >= 1).sum() >= N // 2 and (hd == -1).sum() >= N // 8
    dist, field = nat.shortest_paths(walls, goal, torch.from_numpy(agent).to(device), size,
                                     map_index=torch.from_numpy(index).to(device), field=True)
    assert (dist.cpu().numpy() == hd).all() and (field.cpu().numpy() == hf).all()
    with pytest.raises(nat.MerlinNativeError):
        nat.shortest_paths(walls, goal, torch.from_numpy(agent).to(device), size,
                           map_index=torch.from_numpy(index + 1).to(device))


def test_captured_into_a_graph(device):
    """One kernel on the capturing stream: replayed after a reset on other seeds it equals a fresh eager call, and the
    call changes neither the env's state nor its RNG."""
    env = make_env(device, "hard", 22, max_steps=2)  # every second step resets every env from its look-ahead slot
    env.reset()
    buf = torch.full((N,), -7, dtype=torch.int32, device=device)
    env.optimal_steps(out=buf)  # warm-up
    first = buf.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.optimal_steps(out=buf)
    env.reset(seed=50_000)
    before = env.get_state()
    buf.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    after = env.get_state()
    for k in before:
        assert (before[k] == after[k]).all(), k
    fresh = env.optimal_steps()
    assert torch.equal(buf, fresh) and not torch.equal(buf, first)
    assert (buf.cpu().numpy() == bfs_state(after, range(N))).all()
    # the walk goes on from the same state: the look-ahead slots and the RNG were not touched
    twin = make_env(device, "hard", 22, max_steps=2)
    twin.reset(seed=50_000)
    a = torch.full((N,), 2, dtype=torch.int64, device=device)
    for _ in range(5):
        o1 = env.step(a)[0].clone()
        o2 = twin.step(a)[0]
        assert torch.equal(o1, o2)
    del g
    env.close()
    twin.close()


def test_optimal_paths_and_evaluate_efficiency(device):
    from merlin.actor_critic import CNNActorCritic
    from merlin.pathing import evaluate_efficiency, optimal_paths, optimal_reward

    seeds = list(range(SEED0, SEED0 + 64))
    mixed = optimal_paths(seeds + seeds, difficulty=["easy"] * 64 + ["hard"] * 64, size=16, device=device)
    easy = optimal_paths(seeds, difficulty="easy", size=16, device=device)
    hard = optimal_paths(seeds, difficulty="hard", size=16, device=device)
    assert mixed[0] == easy[0] + hard[0] and mixed[1] == easy[1] + hard[1]
    assert all(isinstance(v, int) for v in mixed[0]) and all(isinstance(v, float) for v in mixed[1])
    assert mixed[1] == optimal_reward(np.array(mixed[0]), 1024).tolist()
    assert np.mean(hard[0]) > np.mean(easy[0]) > 0

    torch.manual_seed(3)
    ac = CNNActorCritic((56, 56, 3), 3).to(device)
    seeds = list(range(SEED0, SEED0 + 32))
    m = evaluate_efficiency(ac, seeds, difficulty="medium", size=8, device=device, max_steps=64)
    pt = m["per_task"]
    assert m["n_tasks"] == 32 and m["n_solvable"] == 32
    assert pt["opt_steps"].tolist() == optimal_paths(seeds, "medium", 8, device, 64)[0]
    assert (pt["steps"][pt["success"]] >= pt["opt_steps"][pt["success"]]).all()
    assert (pt["steps"][~pt["success"]] == 64).all()
    assert 0.0 <= m["spl"] <= m["success_rate"] <= 1.0
    with pytest.raises(ValueError):
        evaluate_efficiency(ac, seeds, difficulty="medium", size=8, device=device, stuck_penalty=True)


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


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    from merlin.actor_critic import CNNActorCritic

    d = tmp_path_factory.mktemp("pathing_cli")
    torch.manual_seed(5)
    torch.save(CNNActorCritic((56, 56, 3), 3).state_dict(), d / "ppo_model_1k.pth")
    (d / "scenario.yaml").write_text(YAML)
    return d


def run_cli(saved, script, args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "ppo-2dgrid_amd", script), "--config",
                        str(saved / "scenario.yaml")] + args, cwd=saved, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_sweep_cli_efficiency(saved):
    args = ["--model_dir", str(saved), "--difficulty", "medium", "--tasks", "8"]
    plain = run_cli(saved, "sweep_checkpoints.py", args)
    assert "spl" not in plain and "success_rate" not in plain and "ppo_model_1k.pth" in plain
    out = run_cli(saved, "sweep_checkpoints.py", args + ["--efficiency"])
    head = [ln for ln in out.splitlines() if ln.startswith("RANK")]
    assert len(head) == 1 and all(c in head[0] for c in ("REWARD", "STEPS", "spl", "success_rate", "reward_ratio"))
    row = [ln for ln in out.splitlines() if ln.startswith("#1")][0].split("|")
    assert len(row) == 7 and "ppo_model_1k.pth" in row[1]
    plain_row = [ln for ln in plain.splitlines() if ln.startswith("#1")][0].split("|")
    assert [c.strip() for c in row[:4]] == [c.strip() for c in plain_row]  # the same ranking figures
    assert 0.0 <= float(row[4]) <= float(row[5]) <= 1.0


def test_analyze_cli_efficiency(saved):
    args = ["--model_path", str(saved / "ppo_model_1k.pth"), "--difficulties", "easy", "medium", "--num_tasks", "8"]
    plain = run_cli(saved, "analyze_distribution.py", args + ["--out", str(saved / "plain.json")])
    res = json.loads((saved / "plain.json").read_text())
    assert "spl" not in plain and all("efficiency" not in res["per_difficulty"][d] for d in ("easy", "medium"))
    out = run_cli(saved, "analyze_distribution.py", args + ["--efficiency", "--out", str(saved / "eff.json")])
    eff = json.loads((saved / "eff.json").read_text())
    assert len([ln for ln in out.splitlines() if " spl " in ln]) == 2
    for d in ("easy", "medium"):
        p = eff["per_difficulty"][d]
        e = p.pop("efficiency")
        assert p == res["per_difficulty"][d]  # everything else as without the flag
        assert "per_task" not in e and len(e["opt_steps"]) == 8 and e["n_tasks"] == 8
        assert {"success_rate", "spl", "excess_steps_mean", "optimal_reward_mean", "reward_ratio", "regret_mean",
                "n_solvable"} <= set(e)
        won = [s for s, r in zip(p["steps"], p["rewards"]) if r > 0]
        assert all(s >= o for s, o, r in zip(p["steps"], e["opt_steps"], p["rewards"]) if r > 0), won
