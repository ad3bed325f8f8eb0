"""GPU: the BENCHED update's gradient pinned to the reference's own gradient at a real minibatch size.

`update_grad_ref.part*.npz` (tests/golden/make_golden.py gen_update_grad) holds the reference PPO.update
(src/ppo.py:122-168) on an 8,192-step single-env rollout of the C oracle's mediumhard env, one epoch of four
minibatches of 2,048, with the FIRST optimizer step recorded whole: the starting weights, every parameter's clipped
gradient as clip_grad_norm_ left it for Adam (:153-156), the pre-clip norm, the parameters' change by that step, and
the normalised advantages / returns the update used.

Here the same inputs run through exactly what bench.py times -- code storage, the HIP GAE, the distinct-frame
grouping, conv2 / conv3 once per receptive-field window, fc1's three GEMMs in h3 form over operand planes (k_h3_pqg /
k_h3_pq / k_h3_tq), the fused loss and the two-launch clip + Adam -- from the reference's starting weights, and the
gradient the benched path hands to its optimizer (p.grad at a ClipAdam.step) is compared tensor by tensor with
the reference's, and both with the same gradient in float64 (the reference's network and loss restated on the CPU in
double, tests/grad64_ref.py).

Conditioning.  At the initial weights the actor's head is tiny (orthogonal init, std 0.01), so the actor tower's and
the actor fc1's gradients are near-cancelling sums (|g| ~ 1e-5 per weight), and a few ReLU pre-activations sit within
fp32 rounding of zero: an fp32 forward that sums in another order may put such a unit on the other side of its kink,
which adds or removes that unit's whole gradient contribution -- ~1e-3 of the actor tower's gradient.  Those ties are
resolved exactly, not allowed for: the float64 restatement returns, for every ReLU unit whose pre-activation is within
2^-21 of its sum's absolute mass (sum |a_k w_k| + |b|), the vector the gradient gains when that unit lands on the
other side (grouped by shared computation: a window, a patch or a distinct frame is evaluated once for all its
samples), a least-squares fit of the difference over those few vectors, rounded to 0 / 1, says which groups flipped,
and what is left after taking them out is held to the plain 1e-5 of the tensor's norm on EVERY tensor.  The old bound
(1e-5 plus the "tie envelope", the summed norms of all the ties' vectors) follows from that and stays asserted.

The advantages: the reference normalises them with fp32 torch moments (src/ppo.py:125), the benched path with f64
moments (the GAE itself is bit-exact); the first test injects the reference's normalised advantages and returns, the
second runs the benched path's own and compares with float64 on those.  The third looks at the 16th optimizer step
(four epochs), where the ratios have left 1 and the clipped branch of the loss is live."""
import numpy as np
import pytest
import torch

from grad64_ref import REL, describe_ties, fixture_frames, grad64, resolve  # REL = 1e-5, on every tensor

pytestmark = pytest.mark.gpu

# the later state: the 16th optimizer step.  At the fixture's learning rate (3e-4) the ratios reach [0.821, 1.164] by
# then and none leaves the clip range [0.8, 1.2], so this test alone runs at 1e-3
EPOCHS_LATER, LR_LATER = 4, 1e-3


def _grad64(g, named, rec, oracle, golden, idx, weights):
    """The float64 gradient (tests/grad64_ref.py) of the fixture rollout's minibatch `idx` at `weights`, on the
    advantages and returns the run used and the fixture's old log-probs."""
    return grad64([n for n, _ in named], weights, fixture_frames(g, oracle, golden), g["actions"], idx,
                  rec["adv_n"], rec["ret"], g["logp"], g["hparams"])


def _tower_ratio(names, grads):
    """|actor-side gradient| / |critic-side gradient| over the towers and fc1 (the heads left out)."""
    n = {k: sum(float(t.double().norm()) ** 2 for nm, t in zip(names, grads)
                if nm.startswith((k + "_extractor.", k + ".0."))) ** 0.5 for k in ("actor", "critic")}
    return n["actor"] / n["critic"]


def _resolved(ref, side, label):
    """Resolve one side's gradient (per tensor, its clip coefficient applied) against the float64 reference `ref`:
    prints the ties with that side's flips; returns (flips, per-tensor remainder, per-tensor raw difference)."""
    diff = [a - b for a, b in zip(side, ref.grads)]
    flips, f, rem = resolve(diff, ref.gdeltas)
    print(f"{label}: groups flipped {[int(k) for k in flips.nonzero()[0]]} of {len(ref.groups)}  "
          f"(fitted f: {', '.join(f'{x:+.3f}' for x in f)})")
    print(describe_ties(ref, flips))
    return flips, rem, diff


def _tensor_ties(ref, i, flips):
    """(ties, groups, flipped groups) among those whose vector reaches tensor i."""
    off = sum(t.numel() for t in ref.grads[:i])
    sl = slice(off, off + ref.grads[i].numel())
    hit = [k for k in range(len(ref.groups)) if bool(ref.gdeltas[k, sl].any())]
    return sum(len(ref.groups[k]) for k in hit), len(hit), [k for k in hit if flips[k]]


def _hold_to_float64(named, ref, ours, label):
    """Every tensor of `ours` within REL of float64 once the flipped tie groups are taken out (and, as before, within
    REL plus the tie envelope as it stands).  Prints the per-tensor table; returns (flips, remainder)."""
    flips, rem, diff = _resolved(ref, ours, label)
    for i, (name, _) in enumerate(named):
        n64 = ref.grads[i].norm().item()
        d64, res = diff[i].norm().item(), rem[i].norm().item()
        ties, groups, flipped = _tensor_ties(ref, i, flips)
        print(f"{name:36s} |g| {n64:.3e}  ties {ties:2d} groups {groups:2d} flipped {flipped}  {label} vs float64: "
              f"unresolved {d64 / n64:.2e}, resolved {res / n64:.2e}  (tie envelope {ref.env[i] / n64:.1e})")
    for i, (name, _) in enumerate(named):
        n64 = ref.grads[i].norm().item()
        assert rem[i].norm().item() <= REL * n64, (name, label, "resolved", rem[i].norm().item() / n64)
        assert diff[i].norm().item() <= REL * n64 + ref.env[i], (name, label, diff[i].norm().item() / n64)
    return flips, rem


def _run(golden, device, ref_adv=False, epochs=None, lr=None, record_at=1):
    """The benched update on the fixture's rollout from the fixture's starting weights.  rec holds the weights, the
    gradient handed to the optimizer, the pre-clip norm and the minibatch's indices at optimizer step `record_at`
    (1-based), and the first step's too.  `epochs` > the fixture's: the further permutations are torch.randperm of a
    seeded CPU generator."""
    from merlin import MerlinVecEnv
    from merlin.ppo import PPO
    from test_gpu_obs_gae import pack

    g = golden("update_grad_ref")
    B, MB, EPOCHS = (int(x) for x in g["cfg"])
    lr0, gamma, lam, clip, vf, ent = (float(x) for x in g["hparams"])
    lr = lr0 if lr is None else lr
    env = MerlinVecEnv(1, "mediumhard", seed=1, device=device)
    perms = [p for p in torch.from_numpy(g["perms"])]
    if epochs is not None:
        gen = torch.Generator().manual_seed(20260)
        perms += [torch.randperm(B, generator=gen) for _ in range(epochs - EPOCHS)]
        EPOCHS = epochs
    torch.manual_seed(0)
    agent = PPO(env, lr=lr, gamma=gamma, lam=lam, clip_eps=clip, update_epochs=EPOCHS, batch_size=B,
                minibatch_size=MB, vf_coef=vf, ent_coef=ent, device=device, perm_fn=lambda n, e: perms[e])
    assert agent.conv1_from_codes and agent.dedup and agent.windows and agent.fast_step
    assert agent.ac.fc1_impl == "h3" and agent._clip_adam is not None
    for (k, t), (s, a, first) in zip(agent.ac.state_dict().items(), g["sums0"]):
        assert abs(t.double().sum().item() - s) <= 1e-5 * max(1.0, abs(a)), k  # the same init (up to LAPACK rounding)
    with torch.no_grad():  # the reference's exact starting weights (its orthogonal_ init ran on this container's CPU)
        for i, (_, p) in enumerate(agent.ac.named_parameters()):
            p.copy_(torch.from_numpy(g[f"p0_{i}"]).to(p.device))
    buf = agent.buf
    buf.codes[:B, 0] = torch.from_numpy(pack(g["codes"])).to(device)
    for dst, key, dt in ((buf.actions, "actions", torch.int64), (buf.logprobs, "logp", torch.float32),
                         (buf.values, "values", torch.float32), (buf.rewards, "rewards", torch.float32),
                         (buf.dones, "dones", torch.float32)):
        dst[:, 0] = torch.from_numpy(g[key]).to(device=device, dtype=dt)

    named = list(agent.ac.named_parameters())
    rec = {"steps": 0}
    step_orig = agent._clip_adam.step

    def step_wrap():
        rec["steps"] += 1
        n = rec["steps"]
        if n == 1:
            rec["grads_first"] = [p.grad.detach().clone() for _, p in named]
        if n == record_at:
            rec["p0"] = [p.detach().clone() for _, p in named]
            rec["grads"] = [p.grad.detach().clone() for _, p in named]
            k = (n - 1) % (B // MB)
            rec["idx"] = perms[(n - 1) // (B // MB)][k * MB:(k + 1) * MB].clone()
        norm = step_orig()
        if n == record_at:
            rec["norm"] = float(norm)
            rec["p1"] = [p.detach().clone() for _, p in named]
        return norm

    agent._clip_adam.step = step_wrap
    if ref_adv:  # the reference's normalisation (src/ppo.py:125, fp32 torch on the CPU) of the bit-exact GAE output
        adv_orig = agent._advantages

        def adv_wrap(rewards, values, dones, last_value, *a, **k):
            # the reference's own normalised advantages and returns, as its update computed them (stored in the
            # fixture: torch's fp32 CPU moments round by the host's vector ISA, so they are data, not recomputed)
            _, ret = adv_orig(rewards, values, dones, last_value, *a, **k)
            rec["adv_n"] = torch.from_numpy(g["adv_norm"]).to(ret.device).view_as(ret)
            ret.copy_(torch.from_numpy(g["returns"]).to(ret.device).view_as(ret))
            return rec["adv_n"], ret

        agent._advantages = adv_wrap
    stats = agent.update(float(g["last_value"]))
    rec.setdefault("adv_n", agent.last_adv_normalized)
    rec["ret"] = agent.buf.returns
    assert agent._wstep is not None  # the fast (benched) step ran, not the autograd fallback
    assert rec["steps"] == EPOCHS * (B // MB) and "grads" in rec
    return g, agent, named, rec, stats, (B, MB, lr)


def _step_lr(rec, i, lr):
    return (rec["p1"][i].double() - rec["p0"][i].double()).cpu() / lr


def test_first_step_gradient_matches_reference(golden, oracle, device):
    """The reference's normalised advantages injected: gradient, pre-clip norm and first Adam step as the reference's;
    the epoch's statistics too.  Ours and the reference's fixture gradient are each resolved against float64 (the
    reference is expected to take no flip) and held to REL on every tensor; ours against the reference, both sides'
    flips taken out, to 2 REL."""
    g, agent, named, rec, stats, (B, MB, lr) = _run(golden, device, ref_adv=True)
    assert [n for n, _ in named] == [str(n) for n in g["param_names"]]
    assert agent.last_distinct_frac < 0.75  # the rollout repeats frames (0.52 distinct per sample): grouping exercised
    assert torch.equal(rec["idx"], torch.from_numpy(g["perms"][0][:MB]))
    ref = _grad64(g, named, rec, oracle, golden, rec["idx"], rec["p0"])
    norm_ref = float(g["first_norm"])
    assert abs(rec["norm"] - norm_ref) <= 1e-5 * norm_ref, (rec["norm"], norm_ref)
    coef = min(1.0, 0.5 / (rec["norm"] + 1e-6))  # clip_grad_norm_'s coefficient (1 under the 0.5 norm)
    ours = [t.double().cpu() * coef for t in rec["grads"]]
    theirs = [torch.from_numpy(g[f"grad{i}"]).double() for i in range(len(named))]  # clipped by the reference itself
    print(f"actor-tower / critic-tower gradient norm at the first step: {_tower_ratio(ref.names, ref.grads):.2e}")
    flips_ref, rem_ref = _hold_to_float64(named, ref, theirs, "reference")
    assert not flips_ref.any(), flips_ref.nonzero()[0].tolist()
    flips, rem = _hold_to_float64(named, ref, ours, "ours")
    for i, (name, _) in enumerate(named):
        n64 = ref.grads[i].norm().item()
        d_ref = (ours[i] - theirs[i]).norm().item()
        d_res = (rem[i] - rem_ref[i]).norm().item()  # ours vs the reference, both sides' flips taken out
        print(f"{name:36s} ours vs reference: unresolved {d_ref / n64:.2e}, resolved {d_res / n64:.2e}")
        assert d_res <= 2 * REL * n64, (name, d_res / n64)
        assert d_ref <= 2 * REL * n64 + ref.env[i], (name, d_ref / n64, ref.env[i] / n64)
    # the first Adam step, lr units: g / (|g| + eps) per element -- where the reference gradient is clear of eps
    # (|g| >= 1e-6: a 1e-5 relative error in g moves the step by < 1e-5) it must match the reference's
    for i, (name, _) in enumerate(named):
        st_ref = torch.from_numpy(g[f"step{i}"].astype(np.float64))
        d = (_step_lr(rec, i, lr) - st_ref).abs()
        clear = torch.from_numpy(g[f"grad{i}"]).double().abs() >= 1e-6
        if clear.any():
            assert d[clear].max().item() <= 2e-3, (name, d[clear].max().item())  # (fp16-stored reference step)
        assert d.max().item() <= 2.0 + 1e-3, name  # anywhere: at most a sign flip of a ~eps gradient
    ref_stats = dict(zip([str(k) for k in g["stat_names"]], g["stat_vals"]))
    for k, v in ref_stats.items():  # the whole epoch's statistics (four optimizer steps)
        tol = 2.5 / MB if k == "clipfrac" else 2e-3 * max(1.0, abs(v))
        assert abs(stats[k] - v) <= tol, (k, stats[k], v)


def test_first_step_gradient_with_own_normalisation_matches_float64(golden, oracle, device):
    """The benched path as it runs (its f64-moment normalisation): every tensor within 1e-5 of the float64 gradient
    of its own advantages once the flipped ties are taken out; the distance to the reference's gradient is printed."""
    g, agent, named, rec, stats, (B, MB, lr) = _run(golden, device)
    ref = _grad64(g, named, rec, oracle, golden, rec["idx"], rec["p0"])
    coef = min(1.0, 0.5 / (rec["norm"] + 1e-6))
    ours = [t.double().cpu() * coef for t in rec["grads"]]
    _hold_to_float64(named, ref, ours, "ours")
    for i, (name, _) in enumerate(named):
        gr = torch.from_numpy(g[f"grad{i}"]).double()
        print(f"{name:36s} vs reference {((ours[i] - gr).norm() / gr.norm()).item():.2e}")
    ref_stats = dict(zip([str(k) for k in g["stat_names"]], g["stat_vals"]))
    for k, v in ref_stats.items():
        tol = 2.5 / MB if k == "clipfrac" else 2e-3 * max(1.0, abs(v))
        assert abs(stats[k] - v) <= tol, (k, stats[k], v)


def test_later_step_gradient_matches_float64(golden, oracle, device):
    """The 16th optimizer step of a four-epoch update (the fixture's permutation, then three seeded ones) at learning
    rate LR_LATER, the benched path's own normalisation: the float64 restatement runs at the weights read back from
    the device before that step, with the fixture's log-probs as the old ones, so the ratios are no longer 1.  Every
    tensor within 1e-5 of float64 once the flipped ties are taken out; the share of the minibatch's samples whose
    float64 ratio lies outside [1 - eps, 1 + eps] (zero gradient through the clipped branch) must be non-zero.

    Measured on the MI355X (profiles/r07_grad.log): at the fixture's 3e-4 the ratios stay inside, [0.8207, 1.1641]
    (profiles/r07_grad_lr3e-4.log), so LR_LATER = 1e-3: ratios in [0.7691, 1.2004], 75 of the 2,048 samples (3.66 %)
    outside the clip range; actor-tower / critic-tower gradient norm 2.33e-1 (first step 5.92e-3); 3 ties in 3 groups,
    none flipped; every tensor within 4.7e-7 of float64."""
    g, agent, named, rec, stats, (B, MB, lr) = _run(golden, device, epochs=EPOCHS_LATER, lr=LR_LATER,
                                                    record_at=EPOCHS_LATER * 4)
    clip = float(g["hparams"][3])
    ref = _grad64(g, named, rec, oracle, golden, rec["idx"], rec["p0"])
    outside = ((ref.ratio < 1 - clip) | (ref.ratio > 1 + clip)).double().mean().item()
    print(f"later state: optimizer step {rec['steps']}, lr {lr:g}, pre-clip norm ours {rec['norm']:.6e} float64 "
          f"{ref.norm:.6e}, ratio in [{ref.ratio.min().item():.4f}, {ref.ratio.max().item():.4f}], share of samples "
          f"outside [1 - {clip}, 1 + {clip}]: {outside:.4f} ({int(round(outside * MB))} of {MB})")
    first = [t.double().cpu() for t in rec["grads_first"]]
    print(f"actor-tower / critic-tower gradient norm: first step {_tower_ratio(ref.names, first):.2e}, "
          f"step {rec['steps']} {_tower_ratio(ref.names, ref.grads):.2e}")
    # the pre-clip norm (it sets ours' clip coefficient): | |a| - |b| | <= |a - b|, summed over the per-tensor bounds
    slack = sum((REL * t.norm().item() + e) ** 2 for t, e in zip(ref.grads, ref.env)) ** 0.5 / ref.coef
    assert abs(rec["norm"] - ref.norm) <= slack, (rec["norm"], ref.norm, slack)
    coef = min(1.0, 0.5 / (rec["norm"] + 1e-6))
    ours = [t.double().cpu() * coef for t in rec["grads"]]
    _hold_to_float64(named, ref, ours, "ours")
    assert outside > 0.0, "no ratio left the clip range: the clipped branch is not exercised"
