"""The FOMAML tests' own reference (no test in here): the reference's meta step (src/fomaml.py:110-212) restated
serially, task by task, in plain torch on recorded support / query batches -- compute_loss with a host GAE loop, a
deep copy of the meta policy per task, SGD, clip_grad_norm_, the tasks' query gradients summed and divided by the task
count, the global clip.  tests/test_gpu_fomaml.py holds the eager meta step to it, tests/test_gpu_fomaml_replay.py
the captured and replayed one.

Recording a batch: the tensors FOMAML.collect_trajectory returns are static rollout storage that the next rollout
overwrites, and at the capture step the tensors handed to the inner / outer step are the ones the HIP graph binds.  So
`record` hands the original dict through untouched and keeps clones on the side."""
import copy

import numpy as np
import torch

BATCH_KEYS = ("codes", "act", "logp", "val", "rew", "done", "last_val")


def record(fm, into):
    """Wrap fm.collect_trajectory: every returned batch is passed on as it is, a clone of its tensors is appended to
    `into`.  Returns the unwrapped method (assign it back to stop recording)."""
    orig = fm.collect_trajectory

    def rec(env, params, steps, **kw):
        b = orig(env, params, steps, **kw)
        into.append({k: b[k].clone() for k in BATCH_KEYS})
        return b

    fm.collect_trajectory = rec
    return orig


def serial_loss(model, batch, g, gamma=0.995, lam=0.95):
    """compute_loss (src/fomaml.py:110-156) for task g on the recorded batch."""
    from merlin import _native as nat

    rews = batch["rew"][:, g].cpu().numpy()
    vals = batch["val"][:, g].cpu().numpy()
    dones = batch["done"][:, g].cpu().numpy()
    last_val = float(batch["last_val"][g].item())
    adv = np.zeros_like(rews)
    gae = 0.0
    for t in reversed(range(len(rews))):
        mask = 1.0 - dones[t]
        next_v = last_val if t == len(rews) - 1 else vals[t + 1]
        delta = rews[t] + gamma * next_v * mask - vals[t]
        gae = delta + gamma * lam * mask * gae
        adv[t] = gae
    dev = batch["rew"].device
    adv_t = torch.tensor(adv, dtype=torch.float32, device=dev)
    adv_t = (adv_t - adv_t.mean()) / (adv_t.std() + 1e-8)
    ret_t = (batch["val"][:, g] + adv_t).detach()
    k = len(rews)
    frames = nat.expand_obs(batch["codes"][:k, g].contiguous(), scale=1.0 / 255.0)
    new_logp, entropy, new_vals = model.evaluate(frames, batch["act"][:, g], prescaled=True)
    ratio = torch.exp(new_logp - batch["logp"][:, g])
    surr1 = ratio * adv_t
    surr2 = torch.clamp(ratio, 0.8, 1.2) * adv_t
    return -torch.min(surr1, surr2).mean() + 0.5 * ((new_vals - ret_t) ** 2).mean() - 0.05 * entropy.mean()


def serial_meta_gradient(meta0, support, query, lr_inner):
    """The meta step's gradient (src/fomaml.py:158-210) on the recorded batches, one task after the other: a copy of
    meta0 (the meta policy from before the step) per task, the support loss, clip_grad_norm_(0.5), one SGD(lr_inner)
    step, the query loss' gradient; the sum over tasks / the task count, clipped to 0.5.
    -> (meta: a copy of meta0 with the clipped meta gradient in .grad, the tasks' query losses, the clipped
    gradient's global norm)."""
    G = int(support["rew"].shape[1])
    meta = copy.deepcopy(meta0)
    grads = [torch.zeros_like(p) for p in meta.parameters()]
    qlosses = []
    for g in range(G):
        fast = copy.deepcopy(meta0)
        opt = torch.optim.SGD(fast.parameters(), lr=lr_inner)
        loss = serial_loss(fast, support, g)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(fast.parameters(), max_norm=0.5)
        opt.step()
        ql = serial_loss(fast, query, g)
        fast.zero_grad()
        ql.backward()
        for acc, p in zip(grads, fast.parameters()):
            acc += p.grad
        qlosses.append(ql.item())
    for p, g in zip(meta.parameters(), grads):
        p.grad = g / G
    torch.nn.utils.clip_grad_norm_(meta.parameters(), max_norm=0.5)
    gnorm = torch.sqrt(sum((p.grad ** 2).sum() for p in meta.parameters())).item()
    return meta, qlosses, gnorm


def assert_meta_gradient(fm, avg_loss, meta, qlosses, gnorm):
    """The eager test's bounds: the average query loss to 1e-4 * max(1, |loss|); every parameter's clipped meta
    gradient (left in .grad) to 1e-4 of max(its norm, 1e-3 of the global norm) -- tensors whose gradient is itself a
    near-cancellation (the value-head bias: mean of new_vals - vals - normalised adv) are judged against the global
    gradient norm.
    How much room that leaves, measured at (4, 8, 8) and (4, 48, 48) over 8 seeds x 4 steps, eager and replayed alike:
    every parameter but critic.2.bias 5e-7 .. 4e-6 of its scale.  critic.2.bias 2e-6 .. 8e-5, twice above 1e-4 (1.2e-4,
    1.6e-4): its exact gradient is 0 (the query loss evaluates the weights the rollout acted with, so new_vals = vals,
    and the normalised advantages have mean 0), what both sides hold is the mean difference between two fp32 forward
    passes -- 1e-7, a unit or two in the last place of a value -- against a scale of 1e-3 * 0.5, and which convolution
    algorithm the serial side's conv2d picks moves the figure by as much.  And a ReLU tie: a hidden unit within a
    rounding of 0 for one sample is live on one side and dead on the other, which adds or removes that sample's whole
    contribution to the unit's gradients (seen: one entry of critic.0.bias off by 3.9e-4, 2.7e-2 of the tensor's scale,
    and once 3.9e-3 at k = 48; neither came back when the serial side's convolutions ran another algorithm).  Two such
    steps in about a hundred measured.  The figures are printed before the assertions."""
    rels = {}
    for (n, a), b in zip(fm.meta_policy.named_parameters(), meta.parameters()):
        scale = max(b.grad.norm().item(), 1e-3 * gnorm)
        rels[n] = ((a.grad - b.grad).norm().item()) / scale
    worst = max(rels, key=rels.get)
    print(f"loss {avg_loss:.7f} serial {float(np.mean(qlosses)):.7f}; gradient error / scale: worst {rels[worst]:.3g} "
          f"({worst}), critic.2.bias {rels['critic.2.bias']:.3g}; clipped norm {gnorm:.4f}")
    assert abs(avg_loss - float(np.mean(qlosses))) <= 1e-4 * max(1.0, abs(avg_loss))
    for n, rel in rels.items():
        assert rel < 1e-4, (n, rel)
