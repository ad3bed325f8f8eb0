"""GPU: merlin_episode_loss (csrc/merlin_fewshot.hip, nat.episode_loss) -- the per-episode GAE, advantage
normalisation and loss of src/distribution_over_tasks.py:97-128 -- against a float64 restatement.

n = 5 episodes in a [9][5] buffer, lengths 1, 2, 9, 5, 3; every entry at t >= length is NaN in all four inputs, so a
read past an episode's end would show in its loss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, LENGTHS, GAMMA, LAM = 9, (1, 2, 9, 5, 3), 0.995, 0.95


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(12)
    n = len(LENGTHS)
    x = {k: rs.randn(T, n).astype(np.float32) for k in ("rew", "val", "nlp", "nval")}
    x["nlp"] = -np.abs(x["nlp"])
    valid = np.arange(T)[:, None] < np.array(LENGTHS)[None, :]
    for k in x:
        x[k][~valid] = np.nan
    return x, valid


def _restate(x, i):
    """(loss, advantages, their std) of episode i in float64."""
    L = LENGTHS[i]
    r, v = x["rew"][:L, i].astype(np.float64), x["val"][:L, i].astype(np.float64)
    adv, gae = np.zeros(L), 0.0
    for t in reversed(range(L)):
        mask = 0.0 if t == L - 1 else 1.0  # the value after the episode never enters
        nv = 0.0 if t == L - 1 else v[t + 1]
        gae = r[t] + GAMMA * nv * mask - v[t] + GAMMA * LAM * mask * gae
        adv[t] = gae
    std = adv.std(ddof=1) if L > 1 else 0.0
    adv_n = (adv - adv.mean()) / (std + 1e-8) if L > 1 else np.zeros(L)
    ret = v + adv_n
    loss = -x["nlp"][:L, i].astype(np.float64).mean() + 0.5 * ((x["nval"][:L, i].astype(np.float64) - ret) ** 2).mean()
    return loss, adv, std


def _run(device, x):
    from merlin import _native as nat

    dev = {k: torch.from_numpy(v).to(device) for k, v in x.items()}
    ws = torch.full((T, len(LENGTHS)), float("nan"), dtype=torch.float32, device=device)
    length = torch.tensor(LENGTHS, dtype=torch.int32, device=device)
    loss = nat.episode_loss(dev["rew"], dev["val"], dev["nlp"], dev["nval"], length, GAMMA, LAM, workspace=ws)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), ws.cpu().numpy()


def test_losses_match_float64_restatement(device, case):
    x, valid = case
    loss, ws = _run(device, x)
    assert np.isfinite(loss).all(), loss
    for i, L in enumerate(LENGTHS):
        ref, adv, std = _restate(x, i)
        if L > 1:  # with a smaller std the + 1e-8 would dominate and the comparison would mean nothing
            assert std >= 1e-3, (i, std)
        print(f"episode {i} (length {L}): loss {loss[i]:.7f} ref {ref:.7f} err {abs(loss[i] - ref):.2e} std {std:.3f}")
        assert abs(loss[i] - ref) <= 1e-5 * max(1.0, abs(ref)), (i, loss[i], ref)
        assert np.allclose(ws[:L, i], adv, rtol=1e-5, atol=1e-6)
    # nothing is written past an episode's end either
    assert np.isnan(ws[~valid]).all() and np.isfinite(ws[valid]).all()


def test_one_step_episode(device, case):
    x, _ = case
    loss, _ = _run(device, x)
    i = LENGTHS.index(1)
    lp, v, nv = (float(x[k][0, i]) for k in ("nlp", "val", "nval"))
    assert abs(loss[i] - (-lp + 0.5 * (nv - v) ** 2)) <= 1e-6 * max(1.0, abs(loss[i]))


def test_advantages_equal_the_gae_kernel_bitwise(device, case):
    """The workspace's advantages are nat.gae's bit for bit on the same valid entries (done = 1 at each episode's last
    step, zero bootstrap, the entries past the end zeroed).  nat.gae takes its thread-per-env kernel above 256
    columns, so the 5 episodes are tiled to 320 columns."""
    from merlin import _native as nat

    x, valid = case
    _, ws = _run(device, x)
    n, reps = len(LENGTHS), 64
    last = (np.arange(T)[:, None] == (np.array(LENGTHS) - 1)[None, :]).astype(np.float32)
    tile = lambda a: torch.from_numpy(np.tile(np.nan_to_num(a, nan=0.0), (1, reps))).to(device)  # noqa: E731
    adv, _ = nat.gae(tile(x["rew"]), tile(x["val"]), tile(last), torch.zeros(n * reps, device=device), GAMMA, LAM)
    adv = adv.cpu().numpy()[:, :n]
    assert (adv[valid].view(np.int32) == ws[valid].view(np.int32)).all()


def test_reproducible_and_argument_checks(device, case):
    from merlin import _native as nat

    x, _ = case
    a, b = _run(device, x)[0], _run(device, x)[0]
    assert (a.view(np.int32) == b.view(np.int32)).all()
    z = torch.zeros(T, 5, device=device)
    with pytest.raises(ValueError):
        nat.episode_loss(z, z, z, z[:4], torch.ones(5, dtype=torch.int32, device=device), GAMMA, LAM)
    with pytest.raises(ValueError):
        nat.episode_loss(z, z, z, z, torch.ones(5, dtype=torch.int64, device=device), GAMMA, LAM)
