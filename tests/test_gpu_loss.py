"""GPU: merlin_ppo_loss (csrc/merlin_loss.hip) against the reference's loss formulation
(src/ppo.py:136-150) written in torch with autograd, on minibatches whose samples repeat frames
(the update's distinct-frame evaluation): loss, the five update statistics, and the gradient
with respect to the per-frame logits / values.  Tolerances: fp32 sums in a different order.

The constructed layouts further down (tests/loss_ref.py) put a frame on every seam of the kernel's partition -- the
64-position items, the 256-position blocks, the carry slots and k_ppo_loss_fix's two accumulators -- and hold the
gradients to a float64 restatement under the GEMM tests' rule: no worse than twice torch's fp32 error, floor 1e-6."""
import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu


def _torch_loss(logits, value, inv, actions, lp_old, adv, ret, clip, vf, ent_coef):
    lg, v = logits.index_select(0, inv), value.index_select(0, inv)
    logp_all = lg - lg.logsumexp(-1, keepdim=True)
    probs = torch.softmax(logp_all, -1)
    logp = logp_all.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    entropy = -(torch.clamp(logp_all, min=torch.finfo(torch.float32).min) * probs).sum(-1)
    ratio = torch.exp(logp - lp_old)
    pi_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    v_loss = ((v - ret) ** 2).mean()
    ent = entropy.mean()
    loss = pi_loss + vf * v_loss - ent_coef * ent
    with torch.no_grad():
        kl = (lp_old - logp).mean()
        cf = (torch.abs(ratio - 1.0) > clip).float().mean()
    return loss, torch.stack([pi_loss, v_loss, ent, kl, cf]).double()


@pytest.mark.parametrize("U,n,A,indexed", [(1, 1, 3, False), (1, 3000, 3, True), (37, 500, 3, True), (5000, 131072 // 8, 3, True),
                                           (300, 4000, 7, False)])
def test_ppo_loss_matches_torch(device, U, n, A, indexed):
    from merlin import _native as nat
    from merlin.ppo import _PPOLoss
    from merlin.windows import MinibatchWindows, _frame_csr

    g = torch.Generator(device=device)
    g.manual_seed(U + n)
    # skewed frame multiplicities; every frame has at least one sample
    inv = torch.cat([torch.arange(U, device=device),
                     (torch.rand(n - U, device=device, generator=g) ** 3 * U).long()])[torch.randperm(n, device=device, generator=g)]
    B = 3 * n if indexed else n
    sample_index = torch.randperm(B, device=device, generator=g)[:n] if indexed else None
    actions = torch.randint(0, A, (B,), device=device, generator=g)
    logits = torch.randn(U, A, device=device, generator=g)
    value = torch.randn(U, device=device, generator=g)
    lp_old = torch.log_softmax(logits.index_select(0, inv) + 0.2 * torch.randn(n, A, device=device, generator=g), -1)
    lp_old = lp_old.gather(-1, actions[sample_index if indexed else slice(None)].unsqueeze(-1)).squeeze(-1)
    lp_full = torch.zeros(B, device=device)
    adv = torch.randn(B, device=device, generator=g)
    ret = torch.randn(B, device=device, generator=g)
    si = sample_index if indexed else torch.arange(n, device=device)
    lp_full[si] = lp_old
    lp_full[si[: n // 10]] = lp_old[: n // 10] + 0.5  # some ratios far outside the clip range
    sk, perm = torch.sort(inv, stable=True)
    new = torch.ones(n, dtype=torch.bool, device=device)
    new[1:] = sk[1:] != sk[:-1]
    mb = MinibatchWindows(None, inv, None, perm.to(torch.int32), _frame_csr(torch.nonzero(new).squeeze(1), n))
    clip, vf, ent_coef = 0.2, 0.5, 0.05

    lr = logits.clone().requires_grad_(True)
    vr = value.clone().requires_grad_(True)
    ref_loss, ref_stats = _torch_loss(lr, vr, inv, actions[si], lp_full[si], adv[si], ret[si], clip, vf, ent_coef)
    ref_loss.backward()

    # the kernel adds the heads' biases itself: pass the logits / value without them
    ba = torch.randn(A, device=device, generator=g).requires_grad_(True)
    bc = torch.randn(1, device=device, generator=g).requires_grad_(True)
    lm = (logits - ba.detach()).requires_grad_(True)
    vm = (value - bc.detach()).requires_grad_(True)
    stats = torch.zeros(6, dtype=torch.float64, device=device)
    loss = _PPOLoss.apply(lm, vm, ba, bc, mb, sample_index, actions, lp_full, adv, ret, clip, vf, ent_coef, stats)
    (2.0 * loss).backward()
    torch.testing.assert_close(loss, ref_loss.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[:5], ref_stats, rtol=1e-5, atol=1e-6)
    assert stats[5] == 0
    torch.testing.assert_close(lm.grad, 2.0 * lr.grad, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(vm.grad, 2.0 * vr.grad, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(ba.grad, 2.0 * lr.grad.sum(0), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(bc.grad, 2.0 * vr.grad.sum(0, keepdim=True), rtol=1e-4, atol=1e-6)
    # fixed order: a second call gives the same bits
    l2, d2, v2, _, _ = nat.ppo_loss(logits, value, mb.offs, mb.order, inv, sample_index, actions, lp_full, adv, ret, clip, vf,
                              ent_coef)
    l1, d1, v1, _, _ = nat.ppo_loss(logits, value, mb.offs, mb.order, inv, sample_index, actions, lp_full, adv, ret, clip, vf,
                              ent_coef)
    assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(v1, v2)
    # merlin_ppo_loss_absmax: the same outputs, and the per-output maxima of |dlogits| / |dvalue| (the bound the
    # heads' backward scales dz's planes by) exactly
    gm = torch.zeros(9, dtype=torch.int32, device=device)
    l3, d3, v3, _, _ = nat.ppo_loss(logits, value, mb.offs, mb.order, inv, sample_index, actions, lp_full, adv, ret,
                                    clip, vf, ent_coef, grad_absmax=gm)
    assert torch.equal(l3, l1) and torch.equal(d3, d1) and torch.equal(v3, v1)
    want = torch.zeros(9, dtype=torch.float32, device=device)
    want[:A] = d1.abs().amax(0)
    want[8] = v1.abs().amax()
    assert torch.equal(gm.view(torch.float32), want)


TOL_FLOOR = 1e-6  # tests/test_gpu_gemm.py's floor


def _err(x, x64, den):
    return float(((x.double().cpu() - x64).abs() / den.clamp_min(1e-300)).max())


def _windows(x, device):
    """The case's MinibatchWindows (frame-sorted sample order and CSR offsets), built as the test above does."""
    from merlin.windows import MinibatchWindows, _frame_csr

    inv = x.inv.to(device)
    sk, perm = torch.sort(inv, stable=True)
    new = torch.ones(x.n, dtype=torch.bool, device=device)
    new[1:] = sk[1:] != sk[:-1]
    return MinibatchWindows(None, inv, None, perm.to(torch.int32), _frame_csr(torch.nonzero(new).squeeze(1), x.n))


def _hip_loss(x, mb, device, stats=None, absmax=False):
    """merlin_ppo_loss_absmax on a workspace prefilled with NaN: a carry slot or block partial that is read without
    having been written this call shows as NaN in the outputs."""
    from merlin import _native as nat

    dev = lambda t: None if t is None else t.to(device)  # noqa: E731
    logits, value, ba, bc = dev(x.logits), dev(x.value), dev(x.ba), dev(x.bc)
    si, act, lp, adv, ret = dev(x.sample_index), dev(x.actions), dev(x.lp_old), dev(x.adv), dev(x.ret)
    ws = torch.full((max(int(nat.lib().merlin_ppo_loss_workspace(x.n)), 1),), float("nan"), dtype=torch.float64,
                    device=device)
    dl = torch.full((x.U, x.A), float("nan"), device=device)
    dv = torch.full((x.U,), float("nan"), device=device)
    loss = torch.full((), float("nan"), device=device)
    dba = torch.full((x.A,), float("nan"), device=device) if ba is not None else None
    dbc = torch.full((1,), float("nan"), device=device) if bc is not None else None
    gm = torch.zeros(9, dtype=torch.int32, device=device) if absmax else None
    p = nat.ptr
    nat.check(nat.lib().merlin_ppo_loss_absmax(p(logits), p(value), p(ba), p(bc), x.U, x.A, p(mb.offs), p(mb.order),
                                               p(mb.inv), x.n, p(si), p(act), p(lp), p(adv), p(ret), R.CLIP, R.VF, R.ENT_CASES,
                                               p(dl), p(dv), p(dba), p(dbc), p(loss), p(stats), p(ws), p(gm),
                                               nat.stream_of(logits)),
              "merlin_ppo_loss_absmax")
    torch.cuda.synchronize()
    return loss, dl, dv, dba, dbc, gm


def _torch32(x, device):
    """torch fp32 autograd on the device, on the inputs the kernel gets: (loss, stats f64[5], dlogits, dvalue, dba, dbc)."""
    lg, v = x.logits.to(device).requires_grad_(True), x.value.to(device).requires_grad_(True)
    ba = x.ba.to(device).requires_grad_(True) if x.ba is not None else None
    bc = x.bc.to(device).requires_grad_(True) if x.bc is not None else None
    loss, stats = _torch_loss(lg + ba if ba is not None else lg, v + bc if bc is not None else v, x.inv.to(device),
                              x.s_actions.to(device), x.s_lp_old.to(device), x.s_adv.to(device), x.s_ret.to(device),
                              R.CLIP, R.VF, R.ENT_CASES)
    loss.backward()
    return loss.detach(), stats.detach(), lg.grad, v.grad, None if ba is None else ba.grad, None if bc is None else bc.grad


_LAYOUTS = sorted(R.layouts())


@pytest.mark.parametrize("A", [1, 2, 3, 8])
@pytest.mark.parametrize("layout", _LAYOUTS)
def test_ppo_loss_constructed_layouts_vs_float64(device, layout, A):
    """Frame sizes given as explicit lists (tests/loss_ref.py: single-sample frames at n = 64, 65, 256, 257; frames of
    exactly one item; a mixed list that holds every way a frame can lie across the 64-position items and 256-position
    blocks, with a partial last item, n % 64 == 0 and n % 256 == 0), A = 1 .. MAXA, with and without the heads' biases
    and the sample index, against the float64 restatement: every gradient's error relative to the summed magnitudes
    of its samples' gradients is at most twice that of torch's fp32 autograd on the same device and inputs (floor
    1e-6: tests/test_gpu_gemm.py's rule)."""
    sizes, offs = R.check_layout(layout)  # asserts the seam classes the layout stands for, from the offsets alone
    for with_bias, indexed in ((True, True), (False, False), (True, False), (False, True)):
        x = R.make_inputs(sizes, A, seed=1000 * A + len(sizes), with_bias=with_bias, indexed=indexed)
        ref = R.reference(x)
        margin = R.clip_margin(ref.ratio, R.CLIP)
        assert margin >= R.MARGIN, margin  # the reference and fp32 stand on the same branch for every sample
        assert int((x.s_adv == 0).sum()) >= x.n // 7
        assert float(ref.cond_logits.max()) <= R.COND_MAX  # every output well resolved in fp32 (loss_ref.ENT_CASES)
        mb = _windows(x, device)
        assert torch.equal(mb.offs.cpu().long(), torch.from_numpy(offs))
        stats = torch.zeros(6, dtype=torch.float64, device=device)
        loss, dl, dv, dba, dbc, gm = _hip_loss(x, mb, device, stats=stats, absmax=True)
        t_loss, t_stats, t_dl, t_dv, t_dba, t_dbc = _torch32(x, device)
        tag = f"{layout} A={A} bias={int(with_bias)} index={int(indexed)}"
        pairs = [("dlogits", dl, t_dl, ref.dlogits, ref.den_logits), ("dvalue", dv, t_dv, ref.dvalue, ref.den_value)]
        if with_bias:
            pairs += [("dbias_a", dba, t_dba, ref.dbias_a, ref.den_bias_a),
                      ("dbias_c", dbc, t_dbc.reshape(1), ref.dbias_c, ref.den_bias_c)]
        for name, hip, t32, x64, den in pairs:
            assert torch.isfinite(hip).all(), (tag, name)
            e_hip, e_t = _err(hip, x64, den), _err(t32, x64, den)
            print(f"{tag} {name}: e(hip) {e_hip:.3e} e(torch) {e_t:.3e}")
            assert e_hip <= max(2 * e_t, TOL_FLOOR), (tag, name, e_hip, e_t)
        if A == 1:
            assert (dl == 0).all(), tag
        got = torch.cat([loss.double().reshape(1), stats[:4]]).cpu()
        t32 = torch.cat([t_loss.double().reshape(1), t_stats[:4]]).cpu()
        want = torch.cat([ref.loss.reshape(1), ref.stats[:4]])
        for q, name in enumerate(("loss", "pi_loss", "v_loss", "entropy", "approx_kl")):
            err, bound = abs(float(got[q] - want[q])), max(2 * abs(float(t32[q] - want[q])),
                                                           TOL_FLOOR * float(ref.term_absmean[q]))
            print(f"{tag} {name}: |hip - f64| {err:.3e} |torch - f64| {abs(float(t32[q] - want[q])):.3e}")
            assert err <= bound, (tag, name, err, bound)
        # the clipped count over n, as a quotient (torch's CPU mean) or as a product with 1 / n (its device mean)
        assert float(stats[4]) in (ref.clip_count / x.n, ref.clip_count * (1.0 / x.n)), (tag, float(stats[4]))
        assert float(stats[5]) == 0.0
        want_max = torch.zeros(9, dtype=torch.float32, device=device)
        want_max[:A] = dl.abs().amax(0)
        want_max[8] = dv.abs().amax()
        assert torch.equal(gm.view(torch.float32), want_max), tag
        again = _hip_loss(x, mb, device, absmax=True)
        for a, b in zip((loss, dl, dv, dba, dbc, gm), again):
            assert (a is None and b is None) or torch.equal(a, b), tag


@pytest.mark.parametrize("n", [64, 65, 256, 257])
def test_ppo_loss_single_sample_frames_permute_bitwise(device, n):
    """Frames of one sample involve no summation: a permutation of the samples (and so of the lanes, items and blocks
    they fall on) permutes dlogits / dvalue bit for bit."""
    sizes, _ = R.check_layout("singles%d" % n)
    x = R.make_inputs(sizes, 3, seed=n, with_bias=True, indexed=False)
    # sample i reads frame i; then sample i is what sample pi[i] was, frame and all
    order = torch.argsort(x.inv)
    for k in ("s_actions", "s_lp_old", "s_adv", "s_ret"):
        setattr(x, k, getattr(x, k)[order])
    x.actions, x.lp_old, x.adv, x.ret, x.inv = x.s_actions, x.s_lp_old, x.s_adv, x.s_ret, torch.arange(n)
    _, dl, dv, _, _, _ = _hip_loss(x, _windows(x, device), device)
    pi = torch.from_numpy(np.random.RandomState(n).permutation(n))
    assert not torch.equal(pi, torch.arange(n))
    for k in ("logits", "value", "actions", "lp_old", "adv", "ret"):
        setattr(x, k, getattr(x, k)[pi])
    _, dl2, dv2, _, _, _ = _hip_loss(x, _windows(x, device), device)
    assert torch.isfinite(dl).all() and torch.isfinite(dv).all()
    assert torch.equal(dl2, dl[pi.to(device)]) and torch.equal(dv2, dv[pi.to(device)])


def test_ppo_loss_stats_accumulate(device):
    """stats[:5] receive the call's means by addition, stats[5] is left alone."""
    sizes, _ = R.check_layout("mixed_partial")
    x = R.make_inputs(sizes, 3, seed=7, with_bias=True, indexed=True)
    mb = _windows(x, device)
    means = torch.zeros(6, dtype=torch.float64, device=device)
    _hip_loss(x, mb, device, stats=means)
    assert (means[:4] != 0).all() and means[4] > 0 and means[5] == 0
    start = torch.tensor([0.5, -2.0, 3.25, 1e-3, 7.0, -11.0], dtype=torch.float64, device=device)
    stats = start.clone()
    _hip_loss(x, mb, device, stats=stats)
    assert torch.equal(stats[:5], start[:5] + means[:5]) and stats[5] == -11.0
    _hip_loss(x, mb, device, stats=stats)
    assert torch.equal(stats[:5], (start[:5] + means[:5]) + means[:5]) and stats[5] == -11.0


def test_ppo_loss_empty_minibatch(device):
    """U = n = 0: the loss is 0, stats keep their bits, no error."""
    from merlin import _native as nat

    z = torch.zeros(0, device=device)
    i64 = torch.zeros(0, dtype=torch.int64, device=device)
    start = torch.tensor([0.5, -2.0, 3.25, 1e-3, 7.0, -11.0], dtype=torch.float64, device=device)
    for si in (None, i64):
        stats = start.clone()
        loss, dl, dv, dba, dbc = nat.ppo_loss(torch.zeros(0, 3, device=device), z,
                                              torch.zeros(1, dtype=torch.int32, device=device),
                                              torch.zeros(0, dtype=torch.int32, device=device), i64, si, i64, z, z, z,
                                              0.2, 0.5, 0.05, stats=stats, bias_actor=torch.ones(3, device=device),
                                              bias_critic=torch.ones(1, device=device))
        torch.cuda.synchronize()
        assert float(loss) == 0.0 and dl.shape == (0, 3) and dv.shape == (0,)
        assert torch.equal(stats.view(torch.int64), start.view(torch.int64))
        assert (dba == 0).all() and (dbc == 0).all()


def test_ppo_loss_bad_action_is_nan(device):
    from merlin import _native as nat

    logits, value = torch.zeros(2, 3, device=device), torch.zeros(2, device=device)
    offs = torch.tensor([0, 1, 2], dtype=torch.int32, device=device)
    order = torch.tensor([0, 1], dtype=torch.int32, device=device)
    actions = torch.tensor([1, 5], device=device)
    z = torch.zeros(2, device=device)
    loss = nat.ppo_loss(logits, value, offs, order, torch.arange(2, device=device), None, actions, z, z + 1, z, 0.2, 0.5, 0.05)[0]
    assert torch.isnan(loss)
