"""GPU: merlin_episode_loss (csrc/merlin_fewshot.hip, nat.episode_loss) -- the per-episode GAE, advantage
normalisation and loss of src/distribution_over_tasks.py:97-128 -- against a float64 restatement.

n = 5 episodes in a [9][5] buffer, lengths 1, 2, 9, 5, 3; every entry at t >= length is NaN in all four inputs, so a
read past an episode's end would show in its loss.  The wide cases at the end run 64, 65 and 200 episodes (one full
block of 64 threads, a second with one live thread, four with the last part-filled) at T = 9 and 70."""
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


def _restate(x, i, lengths=LENGTHS):
    """(loss, advantages, their std) of episode i in float64."""
    L = lengths[i]
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


def _run(device, x, lengths=LENGTHS):
    from merlin import _native as nat

    dev = {k: torch.from_numpy(v).to(device) for k, v in x.items()}
    ws = torch.full(tuple(x["rew"].shape), float("nan"), dtype=torch.float32, device=device)
    length = torch.tensor(lengths, dtype=torch.int32, device=device)
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


def _wide_case(T_, n, ends):
    """n episodes in a [T_][n] buffer: lengths random in 1..T_, the first and the last column and the columns either
    side of every 64-episode block edge forced to ends = (1, T_) or (T_, 1); NaN past every episode's end.  Returns
    (inputs, the same without the NaN, the valid mask, the lengths)."""
    rs = np.random.RandomState(1000 * T_ + n)
    lengths = rs.randint(1, T_ + 1, size=n)
    lengths[0], lengths[-1] = ends
    for b in range(64, n, 64):
        lengths[b - 1], lengths[b] = ends
    x = {k: rs.randn(T_, n).astype(np.float32) for k in ("rew", "val", "nlp", "nval")}
    x["nlp"] = -np.abs(x["nlp"])
    if T_ > T:
        # the advantages' absolute tolerance (1e-6) was set for 9 steps of unit-scale data; the fp32 recurrence's
        # rounding error grows with the steps behind it (up to about 1 / (1 - gamma lam) = 18 of them), and at 70
        # steps the reference's own fp32 op order (oracle.gae_tn on this data) is off by up to 1.4 of that tolerance.
        # A quarter of the scale puts it at 0.4 .. 0.6 of it, where 9 steps of unit scale are (0.2 .. 0.3)
        x["rew"] *= np.float32(0.25)
        x["val"] *= np.float32(0.25)
    valid = np.arange(T_)[:, None] < lengths[None, :]
    full = {k: v.copy() for k, v in x.items()}
    for k in x:
        x[k][~valid] = np.nan
    return x, full, valid, [int(v) for v in lengths]


@pytest.mark.parametrize("ends", ["1,T", "T,1"])
@pytest.mark.parametrize("T_", [9, 70])
@pytest.mark.parametrize("n", [64, 65, 200])
def test_losses_beyond_one_block(device, n, T_, ends):
    """One block of 64 exactly full, a second block with one live thread, four blocks with the last part-filled; the
    shortest and the longest episode on the first and the last column and on both sides of every block edge."""
    x, _, valid, lengths = _wide_case(T_, n, (1, T_) if ends == "1,T" else (T_, 1))
    assert 1 in (lengths[0], lengths[-1]) and T_ in (lengths[0], lengths[-1])
    loss, ws = _run(device, x, lengths)
    assert np.isfinite(loss).all(), loss
    for i, L in enumerate(lengths):
        ref, adv, std = _restate(x, i, lengths)
        if L > 1:  # with a smaller std the + 1e-8 would dominate and the comparison would mean nothing
            assert std >= 1e-3, (i, std)
        assert abs(loss[i] - ref) <= 1e-5 * max(1.0, abs(ref)), (i, L, loss[i], ref)
        assert np.allclose(ws[:L, i], adv, rtol=1e-5, atol=1e-6), (i, L)
    # nothing is written past an episode's end either
    assert np.isnan(ws[~valid]).all() and np.isfinite(ws[valid]).all()
    again, _ = _run(device, x, lengths)
    assert (loss.view(np.int32) == again.view(np.int32)).all()


@pytest.mark.parametrize("n", [65, 200])
def test_length_clamps(device, n):
    """The documented clamps: length 0 gives the one-step loss, length T + 3 the T-step loss, and neither reaches
    outside the [T][n] buffers (the row past the buffer's end does not exist; the rows inside are finite here)."""
    T_ = 9
    _, full, _, lengths = _wide_case(T_, n, (1, T_))
    asked = list(lengths)
    for i in range(n):
        if lengths[i] == 1 and i % 2 == 0:
            asked[i] = 0
        elif lengths[i] == T_:
            asked[i] = T_ + 3
    assert asked[0] == 0 and asked[-1] == T_ + 3 and asked[64] == T_ + 3 and asked != lengths
    want, ws_want = _run(device, full, lengths)
    got, ws_got = _run(device, full, asked)
    assert np.isfinite(want).all()
    assert (got.view(np.int32) == want.view(np.int32)).all()
    assert (ws_got.view(np.int32) == ws_want.view(np.int32)).all()  # NaN where neither wrote
