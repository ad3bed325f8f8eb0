"""GPU: the sampled-policy field's two kernels and what is built on them.

k_policy_chain / k_policy_occupancy against the library's host restatements (a successor-table recursion and scatter,
themselves held to the tests' numpy restatement in test_policy_chain_host.py) at every grid size of
test_gpu_env_sizes' matrix -- all three block sizes: 256 threads up to size 16, 512 at 17, 1,024 at 31 and 32 -- with
M = 9 maps and M = 1, for Dirichlet, constant and one-hot probabilities at horizons 1, 2, 37 and 4 S^2; every output
also requested alone; into guarded buffers; the forward / backward identities on the device outputs; the exact
agreement with k_policy_paths under one-hot probabilities; graph capture; invalid start poses.
Against the real env: 16,384 sampled episodes of one map through k_env_step, which ties the chain's rule to the step
kernel's.  Through the policy: 8,192 episodes sampled by CNNActorCritic.act_codes against sampled_field_for_seeds.

Tolerances (derived): kernel against host 1e-9 (1e-9 T for steps and visits), as test_policy_chain_host.py; Monte
Carlo with N episodes 5 sigma_max / sqrt(N), sigma_max = 0.5 for success and reward (in [0, 1]) and T / 2 for the
length: 0.0195 and 2.81 steps at N = 16,384, T = 144; 0.0276 and 7.07 steps at N = 8,192, T = 256.  The draws are
seeded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from policy_chain_ref import dirichlet_field, reward
from policy_field_ref import CASES, IDS
from test_gpu_policy_field import YAML, dev
from test_policy_chain_host import CHAIN, M9, TOL, _maps, close, horizons, one_hot_identity, prob_fields

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -12345.5


def guarded(n, device):
    """(the whole buffer, its middle n elements): float64, 8-B aligned, 3 guard elements on either side."""
    buf = torch.full((n + 6,), GUARD, dtype=torch.float64, device=device)
    return buf, buf[3:n + 3]


def guards_intact(buf):
    return bool((buf[:3] == GUARD).all()) and bool((buf[-3:] == GUARD).all())


def run_chain(nat, device, w, g, p, size, T, outputs=CHAIN):
    m = w.shape[0]
    bufs = {k: guarded(m * 4 * size * size, device) for k in outputs}
    res = nat.policy_chain(w, g, p, size, T, gamma=0.99, outputs=outputs, out={k: b[1] for k, b in bufs.items()})
    for k, r in zip(CHAIN, res):
        assert (r is not None) == (k in outputs)
        if r is not None:
            assert r.data_ptr() == bufs[k][1].data_ptr() and r.shape == (m, 4, size, size) and guards_intact(bufs[k][0])
    return {k: r.cpu().numpy() for k, r in zip(CHAIN, res) if r is not None}


def run_occupancy(nat, device, w, g, p, a, size, T, outputs=("visits", "hit")):
    m = w.shape[0]
    n = {"visits": m * 4 * size * size, "hit": m * T}
    bufs = {k: guarded(n[k], device) for k in outputs}
    res = nat.policy_occupancy(w, g, p, a, size, T, outputs=outputs, out={k: b[1] for k, b in bufs.items()})
    for k, r in zip(("visits", "hit"), res):
        assert (r is not None) == (k in outputs)
        if r is not None:
            assert r.data_ptr() == bufs[k][1].data_ptr() and guards_intact(bufs[k][0])
    return tuple(None if r is None else r.cpu().numpy() for r in res)


def identities(ch, vis, hit, start, T, what):
    i = (np.arange(len(start)), start[:, 2], start[:, 1], start[:, 0])
    r = np.array([reward(t, T) for t in range(1, T + 1)])
    assert np.abs(hit.sum(1) - ch["success"][i]).max() <= TOL, what
    assert np.abs((hit * r).sum(1) - ch["ret"][i]).max() <= TOL, what
    assert np.abs(vis.sum((1, 2, 3)) - ch["steps"][i]).max() <= TOL * T, what


@pytest.mark.parametrize("diff,size", CASES, ids=IDS)
def test_kernels_vs_host(device, diff, size):
    from merlin import _native as nat

    cells, walls, goal, start = _maps(diff, size)
    start = start.copy()
    start[:, 3] = 0
    w, g, a = dev(walls, device, torch.int32), dev(goal, device), dev(start, device)
    wall = np.broadcast_to((cells == 1)[:, None], (M9, 4, size, size))
    nat.tower_errors(device, raise_on_error=False)
    for name, (probs, action) in prob_fields(diff, size, M9).items():
        p = dev(probs.copy(), device)  # (the shared fields are read-only)
        paths = None if action is None else nat.policy_paths(w, g, dev(action, device), size).cpu().numpy()
        for T in horizons(size):
            want = dict(zip(CHAIN, nat.policy_chain_host(walls, goal, probs, size, T, gamma=0.99)))
            wvis, whit = nat.policy_occupancy_host(walls, goal, probs, start, size, T)
            got = run_chain(nat, device, w, g, p, size, T)
            for k in CHAIN:
                close(got[k], want[k], TOL * T if k == "steps" else TOL, (name, T, k))
            vis, hit = run_occupancy(nat, device, w, g, p, a, size, T)
            close(vis, wvis, TOL * T, (name, T, "visits"))
            close(hit, whit, TOL, (name, T, "hit"))
            assert (vis[wall] == 0).all()
            identities(got, vis, hit, start, T, (name, T))
            if paths is not None:
                one_hot_identity(paths, tuple(got[k] for k in CHAIN), T)
            # M = 1: the last map alone, a grid of one block
            one = run_chain(nat, device, w[-1:], g[-1:], p[-1:].contiguous(), size, T)
            for k in CHAIN:
                assert np.array_equal(one[k], got[k][-1:], equal_nan=True), (name, T, k)
            v1, h1 = run_occupancy(nat, device, w[-1:], g[-1:], p[-1:].contiguous(), a[-1:], size, T)
            assert np.array_equal(v1, vis[-1:]) and np.array_equal(h1, hit[-1:]), (name, T)
        if name == "dirichlet":  # every output alone, the others null
            T = 37
            for k in CHAIN:
                alone = run_chain(nat, device, w, g, p, size, T, outputs=(k,))
                full = run_chain(nat, device, w, g, p, size, T)
                assert list(alone) == [k] and np.array_equal(alone[k], full[k], equal_nan=True), k
            vis, hit = run_occupancy(nat, device, w, g, p, a, size, T)
            assert np.array_equal(run_occupancy(nat, device, w, g, p, a, size, T, outputs=("visits",))[0], vis)
            assert np.array_equal(run_occupancy(nat, device, w, g, p, a, size, T, outputs=("hit",))[1], hit)
    assert nat.tower_errors(device) == 0


def test_invalid_start_pose(device):
    from merlin import _native as nat

    size, T = 11, 37
    cells, walls, goal, start = (x[:4] for x in _maps("mediumhard", size))
    wy, wx = np.argwhere(cells[1, 1:-1, 1:-1] == 1)[0] + 1
    pose = start.copy()
    pose[:, 3] = 0
    pose[1] = (wx, wy, 0, 0)
    pose[2] = (-1, 3, 1, 0)
    probs = prob_fields("mediumhard", size, M9)["dirichlet"][0][:4].copy()
    w, g, p = dev(walls, device, torch.int32), dev(goal, device), dev(probs, device)
    nat.tower_errors(device, raise_on_error=False)
    vis, hit = run_occupancy(nat, device, w, g, p, dev(pose, device), size, T)
    flags = nat.tower_errors(device, raise_on_error=False)
    assert flags & nat.DEVERR_BAD_FRAME
    for i in (1, 2):
        assert np.isnan(vis[i]).all() and np.isnan(hit[i]).all()
    wv, wh = nat.policy_occupancy_host(walls, goal, probs, pose, size, T)
    close(vis, wv, TOL * T, "visits")
    close(hit, wh, TOL, "hit")
    pose[1], pose[2] = start[1], (start[2, 0], start[2, 1], 4, 0)
    pose[:, 3] = 0
    vis, hit = run_occupancy(nat, device, w, g, p, dev(pose, device), size, T)
    assert nat.tower_errors(device, raise_on_error=False) & nat.DEVERR_BAD_FRAME
    assert np.isnan(hit[2]).all() and np.isnan(vis[2]).all() and np.isfinite(hit[[0, 1, 3]]).all()
    with pytest.raises(nat.MerlinNativeError):
        bad = p.clone()
        y, x = np.argwhere(cells[0] != 1)[0]
        bad[0, 1, y, x] = torch.tensor([0.5, -0.1, 0.6], device=device)
        nat.policy_chain(w, g, bad, size, T)
    assert nat.tower_errors(device) == 0


def test_captured_into_a_graph(device):
    """Each kernel captured once on a side stream, as a linear graph, and replayed after the inputs were overwritten:
    the results equal eager calls on the new inputs."""
    from merlin import _native as nat

    size, T = 17, 64
    _, walls, goal, start = _maps("hard", size)
    _, walls2, goal2, start2 = _maps("mediumhard", size)
    start, start2 = start.copy(), start2.copy()
    start[:, 3] = start2[:, 3] = 0
    probs, probs2 = dirichlet_field(M9, size, 1), dirichlet_field(M9, size, 2)
    w, g, p, a = dev(walls, device, torch.int32), dev(goal, device), dev(probs, device), dev(start, device)
    out = {k: torch.zeros((M9, 4, size, size), dtype=torch.float64, device=device) for k in CHAIN}
    occ = {"visits": torch.zeros((M9, 4, size, size), dtype=torch.float64, device=device),
           "hit": torch.zeros((M9, T), dtype=torch.float64, device=device)}
    nat.policy_chain(w, g, p, size, T, out=out)  # warm-up: the device's error word exists
    nat.policy_occupancy(w, g, p, a, size, T, out=occ)
    first = {k: v.clone() for k, v in {**out, **occ}.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            nat.policy_chain(w, g, p, size, T, out=out, validate=False)
            nat.policy_occupancy(w, g, p, a, size, T, out=occ, validate=False)
    w.copy_(dev(walls2, device, torch.int32))
    g.copy_(dev(goal2, device))
    p.copy_(dev(probs2, device))
    a.copy_(dev(start2, device))
    for v in list(out.values()) + list(occ.values()):
        v.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    eager = dict(zip(CHAIN, nat.policy_chain(w, g, p, size, T)))
    eager.update(zip(("visits", "hit"), nat.policy_occupancy(w, g, p, a, size, T)))
    for k, v in {**out, **occ}.items():
        assert torch.equal(torch.nan_to_num(v, nan=-1.0), torch.nan_to_num(eager[k], nan=-1.0)), k
        assert not torch.equal(torch.nan_to_num(v, nan=-1.0), torch.nan_to_num(first[k], nan=-1.0)), k
    want = nat.policy_chain_host(walls2, goal2, probs2, size, T)
    close(out["success"].cpu().numpy(), want[0], TOL, "success")
    assert nat.tower_errors(device) == 0
    del graph


def play(env, obs, T, act):
    """Sampled episodes from the reset that gave `obs`, every env's result frozen at its first done -> (success,
    reward, length) float64[n]."""
    n = env.num_envs
    reward_ = torch.zeros(n, dtype=torch.float64, device=env.device)
    length = torch.zeros(n, dtype=torch.int64, device=env.device)
    won = torch.zeros(n, dtype=torch.bool, device=env.device)
    done = torch.zeros(n, dtype=torch.bool, device=env.device)
    for _ in range(T):
        obs, rew, term, trunc, _ = env.step(act(obs), autoreset=False)
        live = ~done
        fin = live & (term | trunc)
        reward_ = torch.where(fin, rew.double(), reward_)
        won |= live & term
        length += live.long()
        done |= term | trunc
        if bool(done.all()):
            break
    assert bool(done.all())
    env.errors()
    return won.double(), reward_, length.double()


def test_chain_vs_env_rollouts(device):
    """16,384 sampled episodes of one map through the env's own step kernel against the chain at the start pose."""
    from merlin import MerlinVecEnv
    from merlin import _native as nat

    n, size = 16384, 6
    T = 4 * size * size
    env = MerlinVecEnv(n, "mediumhard", size=size, seeds=[1001] * n, device=device)
    assert env.max_steps == T == 144
    probs = dev(dirichlet_field(1, size, 77), device)
    gen = torch.Generator(device=device)
    gen.manual_seed(2024)

    def act(obs):
        _, _, agent = env.snapshot()
        x, y, d = agent[:, 0].long(), agent[:, 1].long(), agent[:, 2].long()
        return torch.multinomial(probs[0, d, y, x], 1, generator=gen).squeeze(1)

    try:
        obs = env.reset().clone()
        walls, goal, agent = env.snapshot()
        assert bool((walls == walls[:1]).all()) and bool((agent == agent[:1]).all())
        w, g, a = walls[:1].contiguous(), goal[:1].contiguous(), agent[:1].contiguous()
        success, ret, steps, _ = nat.policy_chain(w, g, probs, size, T)
        x, y, d = (int(v) for v in a[0, :3])
        want = [float(f[0, d, y, x]) for f in (success, ret, steps)]
        got = [float(v.mean()) for v in play(env, obs, T, act)]
    finally:
        env.close()
    print("chain vs env: predicted", want, "played", got)
    assert 0.05 < want[0] < 0.95, want  # the comparison can fail
    tol = [5 * 0.5 / n ** 0.5, 5 * 0.5 / n ** 0.5, 5 * (T / 2) / n ** 0.5]
    for k, name in enumerate(("success", "reward", "length")):
        assert abs(got[k] - want[k]) <= tol[k], (name, got[k], want[k], tol[k])


MAP_SEED = 1003  # medium 8; a near-uniform policy reaches the goal with probability about 0.85 there


def test_field_vs_sampled_cnn_episodes(device):
    """8,192 episodes sampled by a fresh CNNActorCritic's act_codes against sampled_field_for_seeds' prediction."""
    from merlin import CNNActorCritic, MerlinVecEnv, sampled_field_for_seeds

    n, size = 8192, 8
    torch.manual_seed(11)
    ac = CNNActorCritic((56, 56, 3), 3).to(device)
    field, agent, T = sampled_field_for_seeds(ac, [MAP_SEED], difficulty="medium", size=size, device=device)
    assert T == 256
    want = [float(v[0]) for v in field.at(agent)]
    assert 0.1 <= want[0] <= 0.9, want  # the comparison can fail
    m = field.metrics()
    assert m["n_solvable"] > 0 and 0.0 < m["success_rate"] < 1.0 and np.isfinite(m["value_rmse_sampled"])
    vis, hit = field.occupancy(agent)
    assert abs(float(hit.sum()) - want[0]) <= TOL and abs(float(vis.sum()) - want[2]) <= TOL * T
    env = MerlinVecEnv(n, "medium", size=size, seeds=[MAP_SEED] * n, device=device)
    try:
        with torch.no_grad():
            obs = env.reset().clone()
            assert bool((env.snapshot()[2] == agent).all())  # the field's map and start pose, n times
            got = [float(v.mean()) for v in play(env, obs, T, lambda o: ac.act_codes(o, deterministic=False)[0])]
    finally:
        env.close()
    print("field vs cnn: predicted", want, "played", got)
    tol = [5 * 0.5 / n ** 0.5, 5 * 0.5 / n ** 0.5, 5 * (T / 2) / n ** 0.5]
    for k, name in enumerate(("success", "reward", "length")):
        assert abs(got[k] - want[k]) <= tol[k], (name, got[k], want[k], tol[k])


def test_cli_sampled(device, tmp_path):
    from merlin.actor_critic import CNNActorCritic

    torch.manual_seed(5)
    torch.save(CNNActorCritic((56, 56, 3), 3).state_dict(), tmp_path / "ppo_model_1k.pth")
    (tmp_path / "scenario.yaml").write_text(YAML)
    out_dir = tmp_path / "field"
    r = subprocess.run([sys.executable, os.path.join(REPO, "ppo-2dgrid_amd", "analyze_policy_field.py"), "--config",
                        str(tmp_path / "scenario.yaml"), "--model_path", str(tmp_path / "ppo_model_1k.pth"),
                        "--difficulties", "medium", "--num_tasks", "4", "--base_seed", "4000", "--size", "8",
                        "--out_dir", str(out_dir), "--no_plots", "--sampled"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out_dir)) == ["policy_field.json"]
    res = json.loads((out_dir / "policy_field.json").read_text())
    p = res["per_difficulty"]["medium"]
    assert {"field", "start", "sampled"} <= set(p) and "solved_rate" in p["field"]
    s = p["sampled"]
    assert {"success_rate", "expected_return", "expected_steps", "return_regret", "value_rmse_sampled", "n_solvable",
            "per_map"} <= set(s["field"])
    assert s["field"]["max_steps"] == 48 and s["start"]["seeds"] == list(range(4000, 4004))
    for k in ("success", "ret", "steps"):
        assert len(s["start"][k]) == 4 and all(np.isfinite(v) for v in s["start"][k])
    ld = s["length_distribution"]
    assert len(ld["terminated_at"]) == 48
    assert abs(sum(ld["terminated_at"]) + ld["truncated"] - 1.0) <= 1e-12
    assert abs(sum(ld["terminated_at"]) - np.mean(s["start"]["success"])) <= 1e-12
    assert all(0.0 <= v <= 1.0 for v in s["start"]["success"]) and all(1.0 <= v <= 48.0 for v in s["start"]["steps"])
