"""CPU: the float64 restatement of the minibatch loss (tests/loss_ref.py) that tests/test_gpu_loss.py holds
merlin_ppo_loss to -- against the fp32 torch formulation it restates, against torch's subgradient conventions worked
out by hand, and the constructed layouts against the seam classes they claim."""
import numpy as np
import pytest
import torch

import loss_ref as R
from test_gpu_loss import _torch_loss


def test_equals_the_fp32_formulation():
    """The fp32 `_torch_loss` of the device test on the same inputs, at that test's fp32 tolerances."""
    x = R.make_inputs([3, 1, 70, 200, 1, 25], 5, seed=1, with_bias=False, indexed=False)
    ref = R.reference(x, ent_coef=R.ENT)
    lg, v = x.logits.clone().requires_grad_(True), x.value.clone().requires_grad_(True)
    loss, stats = _torch_loss(lg, v, x.inv, x.actions, x.lp_old, x.adv, x.ret, R.CLIP, R.VF, R.ENT)
    loss.backward()
    torch.testing.assert_close(loss.detach().double(), ref.loss, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats, ref.stats, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lg.grad.double(), ref.dlogits, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(v.grad.double(), ref.dvalue, rtol=1e-4, atol=1e-7)
    assert ref.clip_count == int((torch.abs(ref.ratio - 1.0) > R.CLIP).sum()) and 0 < ref.clip_count < ref.n
    assert R.clip_margin(ref.ratio, R.CLIP) >= 0.049


def test_biases_enter_as_a_sum():
    x = R.make_inputs([3, 1, 70], 4, seed=2, with_bias=True, indexed=True)
    a = R.reference(x, ent_coef=R.ENT)
    b = R.loss64(x.logits.double() + x.ba.double(), x.value.double() + x.bc.double(), x.inv, x.s_actions, x.s_lp_old,
                 x.s_adv, x.s_ret, R.CLIP, R.VF, R.ENT)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.dlogits, b.dlogits) and torch.equal(a.dvalue, b.dvalue)
    torch.testing.assert_close(a.dbias_a, a.dlogits.sum(0), rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(a.dbias_c, a.dvalue.sum().reshape(1), rtol=1e-12, atol=1e-300)
    # the indexed arrays hold the per-sample values at sample_index
    assert torch.equal(x.actions[x.sample_index], x.s_actions) and torch.equal(x.adv[x.sample_index], x.s_adv)


def test_den_is_the_sum_of_the_single_sample_gradient_magnitudes():
    x = R.make_inputs([2, 1, 4], 3, seed=3, with_bias=True, indexed=False)
    ref = R.reference(x, ent_coef=R.ENT)
    den_l, den_v = torch.zeros(x.U, x.A, dtype=torch.float64), torch.zeros(x.U, dtype=torch.float64)
    z, vv = x.logits.double() + x.ba.double(), x.value.double() + x.bc.double()
    for i in range(x.n):  # sample i alone, its share 1 / n of the means
        lg, v = z.clone().requires_grad_(True), vv.clone().requires_grad_(True)
        sel = torch.tensor([i])
        loss, _ = _torch_loss(lg, v, x.inv[sel], x.actions[sel], x.lp_old[sel].double(), x.adv[sel].double(),
                              x.ret[sel].double(), R.CLIP, R.VF, R.ENT)
        (loss / x.n).backward()
        den_l += lg.grad.abs()
        den_v += v.grad.abs()
    torch.testing.assert_close(ref.den_logits, den_l, rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(ref.den_value, den_v, rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(ref.den_bias_a, den_l.sum(0), rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(ref.den_bias_c, den_v.sum().reshape(1), rtol=1e-12, atol=1e-300)
    assert (ref.den_logits >= ref.dlogits.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("r,adv,passes", [
    (1.1, 2.0, True), (1.1, -2.0, True), (0.9, 2.0, True), (0.9, -2.0, True),  # inside: s1 == s2, the whole gradient
    (1.3, 2.0, False),   # above, A > 0: min is the clipped branch
    (1.3, -2.0, True),   # above, A < 0: min is ratio * A
    (0.5, 2.0, True),    # below, A > 0: min is ratio * A
    (0.5, -2.0, False),  # below, A < 0: min is the clipped branch
    (1.3, 0.0, False), (0.5, 0.0, False), (1.0, 0.0, False),  # A == 0: no policy gradient on any branch
])
def test_subgradient_conventions(r, adv, passes):
    """One sample, vf = ent = 0: dlogits = -A * ratio * (onehot(a) - p) when the gradient passes, zero otherwise."""
    z = torch.tensor([[0.3, -1.2, 0.7]], dtype=torch.float64)
    a = 1
    logp = torch.log_softmax(z, -1)[0]
    lp_old = logp[a] - np.log(r)
    ref = R.loss64(z, torch.zeros(1), torch.zeros(1, dtype=torch.int64), torch.tensor([a]), lp_old.reshape(1),
                   torch.tensor([adv]), torch.zeros(1), R.CLIP, 0.0, 0.0)
    assert abs(float(ref.ratio) - r) < 1e-12
    onehot = torch.zeros(3, dtype=torch.float64)
    onehot[a] = 1.0
    want = -adv * float(ref.ratio) * (onehot - logp.exp()) if passes else torch.zeros(3, dtype=torch.float64)
    if passes:
        torch.testing.assert_close(ref.dlogits[0], want, rtol=1e-12, atol=1e-15)
        assert adv == 0.0 or float(ref.dlogits.abs().max()) > 0.1
    else:
        assert (ref.dlogits == 0).all()
    clipped = min(max(r, 1 - R.CLIP), 1 + R.CLIP)
    assert abs(float(ref.loss) + min(r * adv, clipped * adv)) < 1e-12
    assert ref.clip_count == int(abs(r - 1) > R.CLIP)


def test_single_action_has_no_logit_gradient():
    x = R.make_inputs([1, 5, 2], 1, seed=4, with_bias=True, indexed=False)
    ref = R.reference(x)
    assert (ref.dlogits == 0).all() and (ref.den_logits == 0).all() and (ref.stats[2] == 0)


@pytest.mark.parametrize("name", sorted(R.layouts()))
def test_layouts_hold_their_seam_classes(name):
    sizes, offs = R.check_layout(name)
    assert offs[-1] == sum(sizes) and (np.diff(offs) >= 1).all()
    x = R.make_inputs(sizes, 8, seed=5, with_bias=True, indexed=True)
    # the frame of sample i, sorted, reproduces the offsets; the ratios keep their margin; some advantages are zero
    assert (np.bincount(x.inv.numpy(), minlength=x.U) == np.asarray(sizes)).all()
    ref = R.reference(x)
    assert R.clip_margin(ref.ratio, R.CLIP) >= 0.049
    assert int((x.s_adv == 0).sum()) >= x.n // 7
    # every output is well resolved in fp32 (loss_ref.ENT_CASES)
    assert float(ref.cond_logits.max()) <= R.COND_MAX
    assert float(x.logits.double().add(x.ba.double()).softmax(-1).index_select(0, x.inv).gather(
        -1, x.s_actions.unsqueeze(-1)).max()) <= R.P_MAX


def test_seam_classes_by_hand():
    assert R.seam_classes(R.offsets([64, 64])) == {"one_item"}
    assert R.seam_classes(R.offsets([63, 2, 63])) == {"two_straddle", "span1", "ends_on_item_last"}
    assert "block_edge" in R.seam_classes(R.offsets([255, 2])) and "block_edge" not in R.seam_classes(R.offsets([191, 2]))
    assert "aligned_span" in R.seam_classes(R.offsets([128])) and "span1" in R.seam_classes(R.offsets([128]))
    assert R.seam_classes(R.offsets([1, 62, 1])) == {"single", "inside", "ends_on_item_last"}
    assert "span_odd" in R.seam_classes(R.offsets([1, 320])) and "span_even" in R.seam_classes(R.offsets([1, 256]))
