"""The gradient tests' own reference (no test in here, no GPU code): the reference's CNNActorCritic (src/actor_critic.py:
three convs + ReLU per tower, Linear(576, 512) + ReLU, the heads) and PPO loss (src/ppo.py:130-150) restated in float64
on the CPU with F.conv2d / F.linear, and the exact resolution of ReLU ties.

A ReLU pre-activation z = sum_k a_k w_k + b is a TIE at fp32 precision when |z| <= TIE * (sum_k |a_k w_k| + |b|):
within ~log2(K) units of fp32 rounding of the sum's absolute mass, where an fp32 forward that sums in another order may
round it to the other side of zero.  The forward value then changes by |z| ~ 0 only, but the unit's derivative
switches, and the gradient gains exactly

    delta_i = sigma_i * c_i * coef * dz_i/dtheta      (over all parameters; c_i = dL/dh_i, sigma_i = +1 if float64 has
                                                       the unit off (z <= 0), -1 if on; coef the clip coefficient)

The benched path computes a window, a patch or a distinct frame once for every sample that shares it, so ties that
share layer and channel and have bitwise-equal float64 z and input are one computation: they form one GROUP, whose
vector is the sum of its members'.  `resolve` then explains a gradient difference r = g - g64 as a 0/1 combination
of the group vectors (least squares, rounded) and returns what is left, which the tests hold to the plain 1e-5."""
import struct
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

REL = 1e-5  # per-tensor relative norm of the gradient difference once the flipped ties are taken out
TIE = 2.0 ** -21


class _Stop(Exception):
    def __init__(self, z):
        self.z = z


def flat(tensors):
    """Per-tensor list -> one float64 vector (parameter order)."""
    return torch.cat([t.detach().double().reshape(-1).cpu() for t in tensors])


def unflat(vec, like):
    out, off = [], 0
    for t in like:
        out.append(vec[off:off + t.numel()].reshape(t.shape))
        off += t.numel()
    return out


def fixture_frames(g, oracle, golden):
    """The fixture rollout's rendered frames, uint8 [B, 56, 56, 3]."""
    return torch.from_numpy(oracle.render(g["codes"], golden("atlas")["atlas"]))


def grad64(names, weights, frames, actions, idx, adv, ret, old_logp, hparams):
    """The loss gradient of the minibatch `idx` in float64 at `weights` (one tensor per name in `names`, any dtype or
    device); frames uint8 [B, 56, 56, 3], actions / adv / ret / old_logp over the whole batch [B] (indexed by idx
    here), hparams = (lr, gamma, lam, clip, vf, ent).  Returns a namespace:

      grads   per tensor, clip coefficient applied (what clip_grad_norm_ leaves for Adam)
      norm, coef   the pre-clip norm and clip_grad_norm_(0.5)'s coefficient
      ratio   exp(new_logp - old_logp) per sample of the minibatch
      ties    one dict per tie unit: layer, sample (position in idx), channel, pos (index within the channel), z, mass,
              c (dL/dh), on (float64 has z > 0), group
      deltas  [ties, P] float64: delta_i as above;  groups: list of member lists;  gdeltas [groups, P]
      env     per tensor, the old tie envelope: the sum over ties of |delta_i restricted to the tensor|"""
    idx = torch.as_tensor(idx).cpu().long()
    x_all = frames[idx].double().permute(0, 3, 1, 2) / 255.0
    P = {n: w.detach().double().cpu().clone().requires_grad_(True) for n, w in zip(names, weights)}
    plist = list(P.values())

    def net(x, stop=None):
        """(logits, values, [(key, z, h, mass, input, conv kwargs)]); with `stop`, raises _Stop(z) at that layer."""
        acts = []

        def relu(op, a, w, b, key, **kw):
            z = op(a, w, b, **kw)
            if key == stop:
                raise _Stop(z)
            with torch.no_grad():  # the sum's absolute mass, for the tie test
                mass = op(a.abs(), w.abs(), b.abs(), **kw)
            h = torch.relu(z)
            acts.append((key, z, h, mass, a.detach(), (w.shape[-1], kw.get("stride"))))
            return h

        def tower(pre):
            w = lambda i: (P[f"{pre}.network.{i}.weight"], P[f"{pre}.network.{i}.bias"])  # noqa: E731
            h = relu(F.conv2d, x, *w(0), pre + ".0", stride=4)
            h = relu(F.conv2d, h, *w(2), pre + ".2", stride=2)
            h = relu(F.conv2d, h, *w(4), pre + ".4", stride=1)
            return h.flatten(1)

        ha = relu(F.linear, tower("actor_extractor"), P["actor.0.weight"], P["actor.0.bias"], "actor.0")
        hc = relu(F.linear, tower("critic_extractor"), P["critic.0.weight"], P["critic.0.bias"], "critic.0")
        logits = F.linear(ha, P["actor.2.weight"], P["actor.2.bias"])
        values = F.linear(hc, P["critic.2.weight"], P["critic.2.bias"]).squeeze(-1)
        return logits, values, acts

    logits, values, acts = net(x_all)
    lg = torch.log_softmax(logits, -1)
    act = torch.as_tensor(actions).cpu().long().reshape(-1)[idx]
    new_logp = lg.gather(1, act[:, None]).squeeze(1)
    entropy = -(lg.exp() * lg).sum(-1)
    old = torch.as_tensor(old_logp).double().cpu().reshape(-1)[idx]
    a_mb = torch.as_tensor(adv).double().cpu().reshape(-1)[idx]
    r_mb = torch.as_tensor(ret).double().cpu().reshape(-1)[idx]
    lr, gamma, lam, clip, vf, ent = (float(v) for v in hparams)
    ratio = torch.exp(new_logp - old)
    pi = -torch.min(ratio * a_mb, torch.clamp(ratio, 1 - clip, 1 + clip) * a_mb).mean()
    loss = pi + vf * ((values - r_mb) ** 2).mean() - ent * entropy.mean()
    outs = torch.autograd.grad(loss, plist + [a[2] for a in acts])
    grads = list(outs[:len(P)])
    dh = {a[0]: d for a, d in zip(acts, outs[len(P):])}
    norm = float(torch.sqrt(sum((t ** 2).sum() for t in grads)))
    coef = min(1.0, 0.5 / (norm + 1e-6))

    ties, deltas, keys = [], [], {}
    for key, z, _, mass, a, (k, stride) in acts:
        zz = z.detach()
        per = zz.numel() // zz.shape[0]
        for j in torch.nonzero((zz.abs() <= TIE * mass).reshape(-1)).reshape(-1).tolist():
            c = float(dh[key].reshape(-1)[j])
            if c == 0.0:
                continue
            s, u = j // per, j % per  # the unit's sample and its index within the sample
            try:
                net(x_all[s:s + 1], stop=key)
            except _Stop as e:
                zj = e.z.reshape(-1)[u]
            dz = torch.autograd.grad(zj, plist, allow_unused=True)
            zv = float(zz.reshape(-1)[j])
            on = zv > 0.0
            d = flat([torch.zeros_like(p) if t is None else t for t, p in zip(dz, plist)]) * ((-c if on else c) * coef)
            if zz.dim() == 4:  # a conv unit's input: its receptive field in the layer's input
                ch, pos = u // (zz.shape[2] * zz.shape[3]), u % (zz.shape[2] * zz.shape[3])
                oy, ox = pos // zz.shape[3], pos % zz.shape[3]
                field = a[s, :, oy * stride:oy * stride + k, ox * stride:ox * stride + k]
            else:
                ch, pos, field = u, 0, a[s]
            gk = (key, ch, struct.pack("<d", zv), field.contiguous().numpy().tobytes())
            grp = keys.setdefault(gk, len(keys))
            ties.append(dict(layer=key, sample=s, channel=ch, pos=pos, z=zv, mass=float(mass.reshape(-1)[j]), c=c,
                             on=on, group=grp))
            deltas.append(d)
    n_par = sum(p.numel() for p in plist)
    deltas = torch.stack(deltas) if deltas else torch.zeros((0, n_par), dtype=torch.float64)
    groups = [[i for i, t in enumerate(ties) if t["group"] == k] for k in range(len(keys))]
    gdeltas = (torch.stack([deltas[m].sum(0) for m in groups]) if groups
               else torch.zeros((0, n_par), dtype=torch.float64))
    env = [0.0] * len(plist)
    for d in deltas:
        for i, t in enumerate(unflat(d, plist)):
            env[i] += float(t.norm())
    return SimpleNamespace(names=list(names), grads=[t * coef for t in grads], norm=norm, coef=coef,
                           ratio=ratio.detach(), ties=ties, deltas=deltas, groups=groups, gdeltas=gdeltas, env=env)


def resolve(r, gdeltas):
    """r: a gradient difference g - g64, per tensor; gdeltas [groups, P].  Least squares min_f |r - sum_k f_k delta_k|
    in float64 (columns scaled to unit norm for conditioning, the solution unscaled), every f_k rounded to 0 or 1.
    Returns (flips: bool per group, fitted f per group, remainder r - sum_k round(f_k) delta_k per tensor)."""
    rv = flat(r)
    if gdeltas.shape[0] == 0:
        return np.zeros(0, dtype=bool), np.zeros(0), [t.detach().double().cpu() for t in r]
    A = gdeltas.numpy().T
    scale = np.linalg.norm(A, axis=0)
    scale[scale == 0.0] = 1.0
    f = np.linalg.lstsq(A / scale, rv.numpy(), rcond=None)[0] / scale
    flips = f > 0.5
    rem = rv - torch.from_numpy(A[:, flips].sum(1))
    return flips, f, unflat(rem, r)


def describe_ties(ref, flips=None):
    """One line per tie, with its group and (given the resolved flips of one side) whether the group flipped."""
    lines = [f"float64 reference: {len(ref.ties)} ReLU ties at fp32 precision (|z| <= 2^-21 of the sum's absolute "
             f"mass) in {len(ref.groups)} groups"]
    for i, t in enumerate(ref.ties):
        fl = "" if flips is None else ("  FLIPPED" if flips[t["group"]] else "  kept")
        lines.append(f"  tie {i:3d} group {t['group']:3d} {t['layer']:26s} sample {t['sample']:5d} channel "
                     f"{t['channel']:4d} pos {t['pos']:3d}  z {t['z']:+.3e} ({'on' if t['on'] else 'off'})  mass "
                     f"{t['mass']:.3e}  dL/dh {t['c']:+.3e}  |delta| {float(ref.deltas[i].norm()):.3e}{fl}")
    return "\n".join(lines)
