"""The loss tests' own reference (no test in here, no GPU code): the reference's minibatch loss (src/ppo.py:136-150)
restated in float64 on the CPU with torch autograd, over frames whose samples repeat (sample i reads frame inv[i]) --
the formulation of `_torch_loss` in tests/test_gpu_loss.py, in double -- and the constructed frame layouts that
tests/test_gpu_loss.py runs on the device and tests/test_loss_ref.py vets on the CPU.

`loss64` returns, next to the loss, the five statistics and the gradients per frame, a magnitude per output:

    den[u, j] = sum over the samples i of frame u of |g_ij|,   g_ij = the float64 gradient of sample i alone

(for a bias gradient the sum runs over every sample).  An fp32 evaluation that forms each g_ij to a relative error
delta and adds them in any order is within about (delta + depth * 2^-24) * den of the float64 sum, so
|x - x64| / den is the scale-free error the GEMM tests use (there: |C - C64| / sum_k |a_k b_k|).

Subgradients are torch's, which csrc/merlin_loss.hip documents as its own: torch.min sends half of the gradient to
each operand on a tie, torch.clamp passes it inside [lo, hi] (edges included) only.  So with the ratio inside the clip
range s1 == s2 and the whole gradient passes; outside, it is zero exactly when the clipped branch is the minimum."""
from types import SimpleNamespace

import numpy as np
import torch

ITEM, BLOCK = 64, 256  # csrc/merlin_loss.hip: positions per wave item, positions per 256-thread block
RATIOS = (0.5, 0.75, 0.9, 1.0, 1.1, 1.15, 1.3, 2.0)  # each at least 0.05 from 1 +- 0.2
CLIP, VF, ENT = 0.2, 0.5, 0.05
MARGIN = 1e-3  # smallest distance of a float64 ratio to a clip edge that the device cases accept
# The device cases' entropy coefficient and conditioning.  An fp32 evaluation of one sample's gradient is off by a few
# units of 2^-24 of the MASS of its terms, mass_ij = |dla_i| (onehot_j + p_ij) + ent / n p_ij (|logp_ij| + H_i); den
# holds |g_ij|, so an output is resolved to about 2^-23 * cond, cond[u, j] = sum_i mass_ij / den[u, j].  With
# ent = 0.05 and random inputs the policy and the entropy part of a sample cancel at some entries (cond in the
# thousands; a sample with A = 0 or a clipped ratio keeps the entropy part alone, p_j (logp_j + H), which changes
# sign over j): there torch's fp32 autograd and the kernel are both off by 1e-5 .. 2e-3 of den and which of the two
# is closer is chance (measured on the MI355X with ent = 0.05: e(hip) / e(torch) between 0.3 and 1.6 on 125 of 128
# case x option combinations, 2.1, 3.8 and 7.6 on three).  The device cases therefore run with ent = 0 (the entropy
# statistic is still checked; tests/test_gpu_loss.py's random-layout test keeps ent = 0.05) and draw every action
# among those with p <= P_MAX, which bounds cond by (1 + P_MAX) / (1 - P_MAX) = 4: about 5e-7, under the 1e-6 floor.
ENT_CASES, P_MAX, COND_MAX = 0.0, 0.6, 4.0


def _d(t):
    return t.detach().double().cpu()


def loss64(logits, value, inv, actions, lp_old, adv, ret, clip, vf, ent_coef, bias_a=None, bias_c=None):
    """logits [U, A], value [U] (without the heads' biases when those are given), inv int64 [n] (the frame of sample
    i), actions / lp_old / adv / ret [n] per sample; any float dtype, any device.  Everything is evaluated in float64
    from the values as given.  Returns a namespace of CPU float64 tensors:

      loss, stats [5] (pi_loss, v_loss, entropy, approx_kl, clipfrac), clip_count (int), n
      term_absmean [5]   mean |per-sample term| of the loss and of the first four statistics
      dlogits [U, A], dvalue [U], dbias_a [A], dbias_c [1]   (the bias gradients also without biases: the column sums)
      den_logits [U, A], den_value [U], den_bias_a [A], den_bias_c [1]
      cond_logits [U, A]   sum_i mass_ij / den_logits (1 where den is 0), see ENT_CASES
      ratio [n]"""
    lg0, v0 = _d(logits).requires_grad_(True), _d(value).requires_grad_(True)
    U, A = lg0.shape
    inv, actions = inv.detach().cpu().long(), actions.detach().cpu().long()
    n = int(inv.numel())
    ba = (_d(bias_a) if bias_a is not None else torch.zeros(A, dtype=torch.float64)).requires_grad_(True)
    bc = (_d(bias_c).reshape(1) if bias_c is not None else torch.zeros(1, dtype=torch.float64)).requires_grad_(True)
    lp_old, adv, ret = _d(lp_old), _d(adv), _d(ret)
    # one copy of its frame's outputs per sample: its gradient is that of the sample alone
    lg, v = (lg0 + ba).index_select(0, inv), (v0 + bc).index_select(0, inv)
    lg.retain_grad()
    v.retain_grad()
    logp_all = lg - lg.logsumexp(-1, keepdim=True)
    probs = torch.softmax(logp_all, -1)
    logp = logp_all.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    logp.retain_grad()  # dla_i: the policy part alone (the entropy reads logp_all)
    entropy = -(torch.clamp(logp_all, min=torch.finfo(torch.float32).min) * probs).sum(-1)
    ratio = torch.exp(logp - lp_old)
    pi_term = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv)
    v_term = (v - ret) ** 2
    pi_loss, v_loss, ent = pi_term.mean(), v_term.mean(), entropy.mean()
    loss = pi_loss + vf * v_loss - ent_coef * ent
    loss.backward()
    with torch.no_grad():
        kl_term = lp_old - logp
        clipped = torch.abs(ratio - 1.0) > clip
        count = int(clipped.sum())
        stats = torch.stack([pi_loss, v_loss, ent, kl_term.mean(), torch.tensor(count / n, dtype=torch.float64)])
        term = pi_term + vf * v_term - ent_coef * entropy
        absmean = torch.stack([t.abs().mean() for t in (term, pi_term, v_term, entropy, kl_term)])
        gl, gv = lg.grad.abs(), v.grad.abs()
        den_logits = torch.zeros(U, A, dtype=torch.float64).index_add_(0, inv, gl)
        den_value = torch.zeros(U, dtype=torch.float64).index_add_(0, inv, gv)
        onehot = torch.zeros(n, A, dtype=torch.float64).scatter_(1, actions.unsqueeze(-1), 1.0)
        mass = logp.grad.abs().unsqueeze(-1) * (onehot + probs) \
            + abs(ent_coef) / n * probs * (logp_all.abs() + entropy.abs().unsqueeze(-1))
        mass = torch.zeros(U, A, dtype=torch.float64).index_add_(0, inv, mass)
        cond = torch.where(den_logits > 0, mass / den_logits.clamp_min(1e-300), torch.ones_like(mass))
    return SimpleNamespace(loss=loss.detach(), stats=stats, clip_count=count, n=n, term_absmean=absmean,
                           dlogits=lg0.grad, dvalue=v0.grad, dbias_a=ba.grad, dbias_c=bc.grad,
                           den_logits=den_logits, den_value=den_value, den_bias_a=gl.sum(0), den_bias_c=gv.sum().reshape(1),
                           cond_logits=cond, ratio=ratio.detach())


def clip_margin(ratio, clip):
    """Smallest distance of a ratio to either clip edge."""
    return float(torch.minimum((ratio - (1 - clip)).abs(), (ratio - (1 + clip)).abs()).min())


# ----------------------------------------------------------------------------------------------------------------------
# Frame layouts.  Frame u owns the sorted positions offs[u] .. offs[u + 1] - 1; k_ppo_loss gives one wave the item of
# 64 positions, one block four items, and patches the frames that cross an item edge through two carry slots per item
# (k_ppo_loss_fix: carry[j0][1] + sum carry[j][0], j0 < j <= j1, in two alternating accumulators and a tail).
def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])


def seam_classes(offs):
    """The set of seam classes among the frames of a layout, from its offsets alone."""
    out = set()
    for s, e in zip(offs[:-1], offs[1:]):
        s, e = int(s), int(e)
        j0, j1 = s // ITEM, (e - 1) // ITEM
        if e - s == 1:
            out.add("single")
        if j0 == j1:
            if e - s == ITEM:
                out.add("one_item")            # exactly an item: no carry
            elif s % ITEM and e % ITEM:
                out.add("inside")              # wholly inside an item
            elif s % ITEM and e % ITEM == 0:
                out.add("ends_on_item_last")   # begun inside an item, ends on that item's last position
        else:
            span = j1 - j0
            out.add("span%d" % span if span <= 3 else ("span_odd" if span % 2 else "span_even"))
            if s % ITEM == 0 and e % ITEM == 0:
                out.add("aligned_span")        # first position of an item to the last position of a later one
            if e - s == 2:
                out.add("two_straddle")        # two samples either side of an item edge
        if s // BLOCK != (e - 1) // BLOCK:
            out.add("block_edge")              # crosses a 256-position block edge
    return out


MIXED_CLASSES = {"inside", "ends_on_item_last", "aligned_span", "two_straddle", "span1", "span2", "span3", "span_odd",
                 "span_even", "block_edge"}
# n = 2,185: [0,64) [64,128) whole items; 63 inside; 2 straddle 191|192; 63 end on 255; 128 aligned over two items;
# 191 over three items and the block edge 512 (span 2); 320 over six (span 5); 700 over twelve (span 11); 250 over
# four (span 3); 330 over seven (span 6)
MIXED = [64, 64, 63, 2, 63, 128, 1, 191, 1, 320, 5, 700, 3, 250, 330]


def layouts():
    """name -> (frame sizes, the classes the layout must contain, the condition on n it stands for)."""
    out = {}
    for n in (64, 65, 256, 257):
        out["singles%d" % n] = ([1] * n, {"single"}, lambda m, n=n: m == n)
    out["items64"] = ([64] * 9, {"one_item"}, lambda m: m == 576)  # three blocks, the last with one item
    n0 = sum(MIXED)
    out["mixed_partial"] = (MIXED, MIXED_CLASSES, lambda m: m % ITEM != 0)
    out["mixed_item"] = (MIXED + [-n0 % ITEM], MIXED_CLASSES, lambda m: m % ITEM == 0 and m % BLOCK != 0)
    out["mixed_block"] = (MIXED + [-n0 % BLOCK], MIXED_CLASSES, lambda m: m % BLOCK == 0)
    return out


def check_layout(name):
    """(sizes, offs) of a layout after asserting, from the offsets alone, that it holds what it claims."""
    sizes, classes, cond = layouts()[name]
    offs = offsets(sizes)
    got = seam_classes(offs)
    assert classes <= got, (name, sorted(classes - got))
    assert cond(int(offs[-1])), (name, int(offs[-1]))
    if name.startswith("singles"):
        assert all(s == 1 for s in sizes)
    if name == "items64":
        assert got == {"one_item"}, got  # no frame crosses an item edge: no carry is written or read
    return sizes, offs


def make_inputs(sizes, A, seed, with_bias, indexed):
    """CPU inputs of one device case (fp32 / int64 tensors): frame u has sizes[u] samples, scattered over the sample
    positions by a fixed permutation.  logp_old = fp32(logp64[a] - log r) with r drawn from RATIOS, so the float64
    reference and an fp32 evaluation stand on the same branch of min / clamp for every sample; every seventh
    advantage is exactly zero; actions have p <= P_MAX (see ENT_CASES)."""
    rs = np.random.RandomState(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    U, n = len(sizes), int(sizes.sum())
    inv = torch.from_numpy(np.repeat(np.arange(U), sizes)[rs.permutation(n)])
    f32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))  # noqa: E731
    logits, value = f32(rs.randn(U, A)), f32(rs.randn(U))
    ba = f32(rs.randn(A)) if with_bias else None
    bc = f32(rs.randn(1)) if with_bias else None
    z = logits.double() + (ba.double() if with_bias else 0.0)
    logp_all = torch.log_softmax(z, -1).index_select(0, inv)
    # a random action among those with p <= P_MAX (there is one whenever A >= 2): 1 - p_a stays well resolved
    score = torch.from_numpy(rs.rand(n, A)) + (logp_all.exp() <= P_MAX) * 2.0
    act = score.argmax(-1)
    logp = logp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    r = torch.from_numpy(np.asarray(RATIOS)[rs.randint(0, len(RATIOS), n)])
    lp_old = (logp - torch.log(r)).float()
    adv = f32(rs.randn(n))
    adv[::7] = 0.0
    # returns at a distance of 0.5, 1 or 2 from the value: v + bias - R is not a difference of near-equal numbers
    vb = (value.double() + (bc.double() if with_bias else 0.0)).index_select(0, inv)
    ret = (vb + torch.from_numpy(rs.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], n))).float()
    x = SimpleNamespace(U=U, n=n, A=A, inv=inv, logits=logits, value=value, ba=ba, bc=bc, sample_index=None,
                        actions=act, lp_old=lp_old, adv=adv, ret=ret)
    # per-sample views (what sample i reads) stay in x.s_*; with an index the arrays passed on are 3n long
    x.s_actions, x.s_lp_old, x.s_adv, x.s_ret = act, lp_old, adv, ret
    if indexed:
        B = 3 * n
        si = torch.from_numpy(rs.permutation(B)[:n])
        x.sample_index = si
        x.actions = torch.from_numpy(rs.randint(0, A, B))
        x.lp_old, x.adv, x.ret = f32(rs.randn(B)), f32(rs.randn(B)), f32(rs.randn(B))
        x.actions[si], x.lp_old[si], x.adv[si], x.ret[si] = act, lp_old, adv, ret
    return x


def reference(x, clip=CLIP, vf=VF, ent_coef=ENT_CASES):
    return loss64(x.logits, x.value, x.inv, x.s_actions, x.s_lp_old, x.s_adv, x.s_ret, clip, vf, ent_coef, x.ba, x.bc)
