"""GPU: batched few-shot evaluation (merlin/few_shot.py, merlin.evaluation.evaluate_few_shot, the
distribution_over_tasks.py CLI) against the reference's evaluate_few_shot (tests/golden/fewshot_ref.npz, recorded by
tests/golden/make_fewshot_golden.py from src/distribution_over_tasks.py:132-209), against evaluate_zero_shot, and
against the C oracle's replay of the recorded episodes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, tol=1e-5):
    return abs(a - b) <= tol * max(1.0, abs(b))


def _fixture_batch(fx, step, G, device):
    """Adapt step `step`'s recorded support rollouts as FOMAML's [k][tasks] batch dict (codes packed)."""
    from test_windows import pack

    codes = np.stack([pack(fx[f"t{g}_a{step}_codes"]) for g in range(G)], 1)  # [k + 1, G, 8]
    b = {"codes": torch.from_numpy(codes).to(device)}
    for k in ("act", "rew", "val", "logp", "done"):
        b[k] = torch.from_numpy(np.stack([fx[f"t{g}_a{step}_{k}"] for g in range(G)], 1)).to(device)
    b["last_val"] = torch.tensor([float(fx[f"t{g}_a{step}_last_val"]) for g in range(G)], device=device)
    return b


def test_replays_the_reference_adaptation_and_episode(golden, device):
    """With the fixture's weights: per adapt step the grouped policy at the current per-task weights reproduces the
    recorded logp / value / bootstrap value on the recorded observations (1e-5), adapt_step on the recorded batch
    follows; after both steps adapted - meta agrees per tensor to 1e-4 of its norm (floored at 1e-3 of the task's
    whole delta norm, the scaling of test_gpu_fomaml's fixture test); the deterministic episode gives the recorded
    actions, reward and steps exactly and the recorded loss to 1e-5."""
    from merlin import grouped_policy as gp
    from merlin.actor_critic import CNNActorCritic
    from merlin.few_shot import FewShotAdapter

    fx = golden("fewshot_ref")
    G, S, K, max_steps = (int(v) for v in fx["cfg"])
    torch.manual_seed(0)  # the reference's init order: the same weights
    ac = CNNActorCritic((56, 56, 3), 3)
    for (k, t), (s, a, first) in zip(ac.state_dict().items(), fx["sums0"]):
        t = t.double()
        assert abs(t.sum().item() - s) <= 1e-5 * max(1.0, a) and abs(t.abs().sum().item() - a) <= 1e-6 * max(1.0, a), k
    ac = ac.to(device)
    names = [n for n, _ in ac.named_parameters()]
    assert names == [str(n) for n in fx["names"]]
    ad = FewShotAdapter(ac, lr_inner=float(fx["lr_inner"]), device=device, max_steps=max_steps)
    try:
        params = None
        for step in range(S):
            batch = _fixture_batch(fx, step, G, device)
            cur = ad.meta_params(G) if params is None else params
            rows = batch["codes"].transpose(0, 1).reshape(G * (K + 1), 8).contiguous()
            acts = torch.cat([batch["act"], torch.zeros_like(batch["act"][:1])]).t()
            with torch.no_grad():
                lp, _, v = gp.evaluate(cur, rows, K + 1, acts)
            for name, got, ref in (("logp", lp[:, :K].t(), batch["logp"]), ("val", v[:, :K].t(), batch["val"]),
                                   ("last_val", v[:, K], batch["last_val"])):
                err = ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
                print(f"adapt step {step} {name}: max err {err:.2e}")
                assert err <= 1e-5, (step, name, err)
            params = ad.adapt_step(batch, params)
        for g in range(G):
            stats = fx[f"t{g}_delta_stats"]
            gnorm = float(np.sqrt((stats[:, 0] ** 2).sum()))
            for i, n in enumerate(names):
                d = (params[n][g] - dict(ac.named_parameters())[n].detach()).reshape(-1).double().cpu()
                scale = max(float(stats[i, 0]), 1e-3 * gnorm)
                assert abs(d.norm().item() - float(stats[i, 0])) <= 1e-4 * scale, (g, n)
                sel = fx[f"t{g}_delta_idx"][i]
                sel = sel[sel >= 0]
                err = (d[torch.from_numpy(sel)] - torch.from_numpy(fx[f"t{g}_delta_vals"][i][:sel.size])).abs().max()
                assert err.item() <= 1e-4 * scale, (g, n, err.item(), scale)
        seeds = [int(s) for s in fx["seeds"]]
        rew, steps, loss, acts = ad.episode(params, seeds, max_steps=max_steps, record=True)
        for g in range(G):
            ref_steps = int(fx[f"t{g}_ep_steps"])
            print(f"task {g}: steps {steps[g]} / {ref_steps} reward {rew[g]} / {float(fx[f't{g}_ep_reward'])} "
                  f"loss {loss[g]:.7f} / {float(fx[f't{g}_ep_loss']):.7f} margin {float(fx[f't{g}_ep_margin']):.1e}")
            assert steps[g] == ref_steps
            assert (acts[:ref_steps, g].numpy() == fx[f"t{g}_ep_actions"]).all(), g
            assert rew[g] == float(fx[f"t{g}_ep_reward"])
            assert _close(loss[g], float(fx[f"t{g}_ep_loss"])), (g, loss[g], float(fx[f"t{g}_ep_loss"]))
    finally:
        ad.close()


@pytest.fixture(scope="module")
def policy(device):
    from merlin.actor_critic import CNNActorCritic

    torch.manual_seed(11)
    return CNNActorCritic((56, 56, 3), 3).to(device)


def test_zero_shot_identities(policy, device):
    """adapt_steps = 0 is evaluate_zero_shot, and so are two adapt steps with lr_inner = 0; 5 seeds in chunks of 2
    (three chunks, the last one padded)."""
    from merlin.evaluation import evaluate_few_shot, evaluate_zero_shot

    seeds = list(range(5000, 5005))
    r0, s0, l0 = evaluate_zero_shot(policy, seeds, device=device, max_steps=24)
    r1, s1, l1 = evaluate_few_shot(policy, seeds, 0, device=device, max_steps=24, task_batch=2)
    assert len(r1) == len(s1) == len(l1) == 5
    assert r1 == r0 and s1 == s0
    for a, b in zip(l1, l0):
        print(f"loss {a:.7f} zero-shot {b:.7f}")
        assert _close(a, b), (a, b)
    r2, s2, _ = evaluate_few_shot(policy, seeds, 2, lr_inner=0.0, k_support=8, device=device, max_steps=24,
                                  task_batch=2)
    assert r2 == r0 and s2 == s0


def test_adapted_episodes_match_oracle_replay(policy, oracle, device):
    """The pattern of test_gpu_eval: the adapted policies' recorded episode actions replayed through the C oracle on
    the same seeds end at the same step with the same reward."""
    from merlin.few_shot import FewShotAdapter

    seeds = [1999, 2000, 2001, 2002]
    ad = FewShotAdapter(policy, lr_inner=0.05, device=device, max_steps=24)
    try:
        params = ad.adapt(seeds, 1, 16)
        moved = sum(int((params[n] != p.detach()).any()) for n, p in policy.named_parameters())
        assert moved == len(params)
        rew, steps, loss, acts = ad.episode(params, seeds, record=True)
    finally:
        ad.close()
    assert np.isfinite(loss).all()
    _, orew, oterm, otrunc, _ = oracle.batch_rollout(np.array(seeds, dtype=np.uint64), acts.numpy(),
                                                     difficulty="mediumhard", max_steps=24)
    done = np.maximum(oterm, otrunc).astype(bool)
    for i in range(len(seeds)):
        assert done[:, i].any(), i
        first = int(np.argmax(done[:, i]))
        assert steps[i] == first + 1, (i, steps[i], first + 1)
        assert abs(rew[i] - float(orew[: first + 1, i].astype(np.float64).sum())) <= 1e-6, i


def test_reproducible(policy, device):
    from merlin.evaluation import evaluate_few_shot

    out = []
    for _ in range(2):
        torch.manual_seed(3)
        out.append(evaluate_few_shot(policy, [7, 8, 9], 1, lr_inner=0.05, k_support=16, device=device, max_steps=24,
                                     task_batch=2))
    assert out[0] == out[1]


def test_cli_writes_results(device, tmp_path):
    from merlin.actor_critic import CNNActorCritic

    for k, name in enumerate(("ppo_a", "fomaml_b")):
        torch.manual_seed(20 + k)
        torch.save(CNNActorCritic((56, 56, 3), 3).state_dict(), tmp_path / f"{name}.pth")
    script = os.path.join(REPO, "ppo-2dgrid_amd", "distribution_over_tasks.py")
    res = subprocess.run([sys.executable, script, "--ppo_model", str(tmp_path / "ppo_a.pth"), "--fomaml_model",
                          str(tmp_path / "fomaml_b.pth"), "--num_tasks", "4", "--adapt_steps", "1", "--k_support", "16",
                          "--task_batch", "4", "--out_dir", str(tmp_path / "out")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    path = tmp_path / "out" / "ppo_a_vs_fomaml_b" / "seed_100000" / "1_shot" / "results.json"
    assert path.exists()
    r = json.loads(path.read_text())
    for who in ("ppo", "fomaml"):
        for what in ("rewards", "steps", "losses"):
            assert len(r[f"{who}_{what}"]) == 4 and np.isfinite(r[f"{who}_{what}"]).all(), (who, what)
        assert np.isfinite(r[f"{who}_mean_reward"])
    assert sorted(r["reward_metrics"]) == ["js_div", "kl_ab", "kl_ba", "mean_norm_diff", "wasserstein"]


def test_mlp_policy_is_refused(device):
    from merlin.actor_critic import MLPActorCritic
    from merlin.evaluation import evaluate_few_shot

    with pytest.raises(ValueError, match="CNNActorCritic"):
        evaluate_few_shot(MLPActorCritic(9408, 3).to(device), [1, 2], 1, device=device)
