"""GPU: the optimizer step's weight-only chain as six plain launches (merlin/fast_step.py NATIVE_CHAIN:
merlin_stage_bwd_scatter, merlin_clip_adam_chain, merlin_stage_fwd_planes) against the form it replaces -- the two
captured graphs with torch's index_copy_ / index_select, h3_amax, two h3_split, the zeroings and the norm's add around
merlin_clip_adam.  Every fold does the same operations on the same values in the same order (exact maxima and plain
copies are order-free), so everything is compared bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# the sizes at k_opt_*'s 1024-element block edges; the two 1024-element tensors stand for fc1's weights: "towers"
# [16, 64] of one stacked tensor with a scale word each, in D straight and transposed (two slots per element)
SIZES = (1, 1023, 1024, 1024, 1025, 4097)
TW = (2, 3)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)


def _chain_case(device, gscale, bad=None):
    from merlin import _native as nat

    g = torch.Generator().manual_seed(11)
    n_flat = sum(SIZES)
    flat = (torch.randn(n_flat, generator=g) * 0.05).to(device)
    offs = [sum(SIZES[:i]) for i in range(len(SIZES))]
    idx = [torch.arange(o, o + n) for o, n in zip(offs, SIZES)]
    stacked = torch.stack([idx[TW[0]], idx[TW[1]]]).view(2, 16, 64)
    # D: the small tensors, the stacked pair [2, 16, 64], the last tensor, the pair transposed
    segs = [idx[0], idx[1], idx[4], stacked.reshape(-1), idx[5], stacked.transpose(1, 2).reshape(-1)]
    fwd_map = torch.cat(segs).to(device)
    w_off = SIZES[0] + SIZES[1] + SIZES[4]
    cnt = torch.bincount(fwd_map, minlength=n_flat)
    order = torch.argsort(fwd_map, stable=True)
    first = torch.cumsum(cnt, 0) - cnt
    slots = torch.full((n_flat, 2), -1, dtype=torch.int32, device=device)
    for k in range(2):
        has = cnt > k
        slots[has, k] = order[first[has] + k].to(torch.int32)
    assert int((slots[:, 1] >= 0).sum()) == 2048

    def state(buf):
        ps = [buf[o:o + n] for o, n in zip(offs, SIZES)]
        gg = torch.Generator().manual_seed(12)
        gs = [(torch.randn(n, generator=gg) * gscale).to(device) for n in SIZES]
        if bad is not None:
            gs[4][517] = bad
        ms = [(torch.randn(n, generator=gg) * 1e-3).to(device) for n in SIZES]
        vs = [(torch.rand(n, generator=gg) * 1e-5).to(device) for n in SIZES]
        st = [torch.full((), 3.0, device=device) for _ in SIZES]  # a nonzero step count
        return ps, gs, ms, vs, st

    hyper = (2.5e-4, 0.9, 0.999, 1e-8, 0.5)
    totals0 = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 0.3], dtype=torch.float64)
    # today's sequence
    flat_r = flat.clone()
    ref = state(flat_r)
    am_r = torch.full((16,), 0x41234567, dtype=torch.int32, device=device)
    amw_r = torch.full((2,), 0x7F000000, dtype=torch.int32, device=device)
    tot_r = totals0.to(device)
    norms_r = []
    for _ in range(2):
        norm = nat.clip_adam(*ref, *hyper)
        tot_r[5:].add_(norm.detach())
        am_r.zero_()
        D_r = flat_r.index_select(0, fwd_map)
        nat.h3_amax(D_r[w_off:w_off + 2048].view(2, 1024), out=amw_r)  # (zeroes amw_r first)
        norms_r.append(norm.clone())
    # the chained launches: the scale words start as junk the first launch has to zero, D as NaN
    flat_c = flat.clone()
    new = state(flat_c)
    am_c, amw_c = torch.full_like(am_r, 0x41234567), torch.full_like(amw_r, 0x7F000000)
    tot_c = totals0.to(device)
    D_c = torch.full((fwd_map.numel(),), float("nan"), device=device)
    ps = new[0]
    chain = nat.AdamChain([am_c, amw_c], flat_c, slots, D_c, amax=amw_c, amax_slot={id(ps[TW[0]]): 0, id(ps[TW[1]]): 1},
                          total=tot_c[5:])
    norms_c = [nat.clip_adam(*new, *hyper, chain=chain).clone() for _ in range(2)]
    torch.cuda.synchronize()
    for name, a, b in zip("pgmvs", ref, new):
        for i, (x, y) in enumerate(zip(a, b)):
            assert _same(x, y), (name, i)
    assert _same(D_r, D_c) and _same(tot_r, tot_c)
    assert torch.equal(am_r, am_c) and torch.equal(amw_r, amw_c)
    for x, y in zip(norms_r, norms_c):
        assert _same(x, y)
    return D_c, amw_c


@pytest.mark.parametrize("gscale", [1e-4, 3.0])  # clipping inactive / active
def test_chained_clip_adam_matches_todays_sequence(device, gscale):
    D, amw = _chain_case(device, gscale)
    assert bool(torch.isfinite(D).all()) and int(amw.min()) > 0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_chained_clip_adam_nonfinite_gradient(device, bad):
    """An infinite element turns itself NaN (coefficient 0), a NaN one the norm: every parameter and every D slot."""
    D, _ = _chain_case(device, 3.0, bad=bad)
    assert bool(torch.isnan(D).any()) and (bad == float("inf") or bool(torch.isnan(D).all()))


def test_chained_clip_adam_rejects_a_parameter_off_the_flat_buffer(device):
    from merlin import _native as nat

    flat = torch.zeros(64, device=device)
    p, g, m, v, s = (torch.zeros(8, device=device) for _ in range(5))
    slots = torch.full((64, 2), -1, dtype=torch.int32, device=device)
    with pytest.raises(nat.MerlinNativeError):
        nat.clip_adam([p], [g], [m], [v], [s[:1]], 1e-3, 0.9, 0.999, 1e-8, 0.5,
                      chain=nat.AdamChain([], flat, slots, torch.zeros(64, device=device)))


@pytest.fixture(scope="module")
def stage(device):
    """A native-chain WeightStage over a CNNActorCritic with random weights (the model's own, fixed shapes)."""
    from merlin import CNNActorCritic, fast_step

    assert fast_step.NATIVE_CHAIN
    torch.manual_seed(21)
    ac = CNNActorCritic((56, 56, 3), 3).to(device)
    with torch.no_grad():
        for p in ac.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    flat = fast_step.flatten_parameters(ac)
    fgrad = torch.zeros_like(flat)
    st = fast_step.WeightStage(ac, flat, fgrad, impl="hip", fc1="h3")
    assert st.native
    return st


def test_one_launch_stage_forward(device, stage):
    from merlin import _native as nat

    st = stage
    D = st.flat_params.index_select(0, st.fwd_map)
    W1, b1, W2, W4p, W4pT = (st.seg(D, k) for k in ("W1", "b1", "W2", "W4p", "W4pT"))
    atlas, idx = st.ac.stage_consts(device)[:2]
    HT, T2 = nat.stage_tables_fwd(W1, b1, W2, atlas, idx)
    amax = nat.h3_amax(W4p)
    P4, P4t = nat.h3_split(W4p, amax), nat.h3_split(W4pT, amax)
    st.HT.fill_(float("nan"))
    st.T2.fill_(float("nan"))
    for pl in st._p4:
        pl.fill_(-1)
    st.refresh()
    outs = st.forward()
    torch.cuda.synchronize()
    assert torch.equal(st.D, D) and torch.equal(st.amaxW, amax)
    assert torch.equal(outs[0], T2) and torch.equal(st.HT, HT)
    assert torch.equal(st.planes[0], P4) and torch.equal(st.planes[1], P4t)
    for o, k in zip(outs[1:], ("b2", "W3r", "b3", "W4p", "b4")):
        assert torch.equal(o, st.seg(D, k)), k


def test_fold_scatter_matches_index_copy(device, stage):
    from merlin import _native as nat

    st = stage
    st.refresh()
    st.forward()
    g = torch.Generator(device=device).manual_seed(5)
    for t in st.grads:  # dT2 and the gradients the step writes into DG
        t.copy_(torch.randn(t.shape, device=device, generator=g))
    n = st.n_grad
    is_stage = torch.zeros(st.flat_grad.numel(), dtype=torch.bool, device=device)
    is_stage[st.fwd_map[:n]] = True
    assert 0 < int((~is_stage).sum()) < 4096  # the heads' weights and biases: not the stage's

    def prefill(buf):
        buf[is_stage] = float("nan")
        buf[~is_stage] = 7.25
        return buf

    # the oracle: the plain three launches into a derived-gradient buffer of its own, then torch's scatter
    DG = st.DG.clone()
    atlas, _, koff, kv = st.ac.stage_consts(device)
    nat.stage_tables_bwd(st.seg(st.D, "W2"), st.HT, st.gT2, atlas, koff, kv, dW1=st.seg(DG, "W1"),
                         db1=st.seg(DG, "b1"), dW2=st.seg(DG, "W2"))
    want = prefill(torch.empty_like(st.flat_grad))
    want.index_copy_(0, st.fwd_map[:n], DG[:n])
    prefill(st.flat_grad)
    st.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want[is_stage]).all())
    assert torch.equal(st.flat_grad[is_stage], want[is_stage])
    assert bool((st.flat_grad[~is_stage] == 7.25).all())
    assert torch.equal(st.DG[:n], DG[:n])


def _run(device, monkeypatch, native, between=None, iters=3):
    """tests/test_gpu_fast_step.py::_run's agent with the chain switched; between(agent, i) after update i."""
    from merlin import MerlinVecEnv, fast_step
    from merlin.ppo import PPO

    monkeypatch.setattr(fast_step, "NATIVE_CHAIN", native)
    env = MerlinVecEnv(256, "mediumhard", seed=5, device=device)
    torch.manual_seed(3)
    agent = PPO(env, lr=1e-3, batch_size=256 * 64, minibatch_size=256 * 16, update_epochs=2, ent_coef=0.05,
                device=device)
    stats = []
    for i in range(iters):
        stats.append(agent.update(agent.collect_rollouts()))
        assert agent._wstep is not None and agent._wstep.stage.native == native
        assert (agent._wstep.chain is not None) == native
        if between is not None and i + 1 < iters:
            between(agent, i)
    torch.cuda.synchronize()
    return agent, stats


def _edit(agent, i):  # an in-place edit between two updates: Adam's launches never saw it, the refresh has to
    if i == 0:
        with torch.no_grad():
            agent.ac.actor[0].weight.mul_(1.5)
            agent.ac.critic_extractor.network[2].weight.add_(0.01)


def _rebind(agent, i):  # a parameter moved off the flat buffer: the step re-homes it and builds a new stage
    if i == 1:
        w = agent.ac.actor[0].weight
        w.data = w.data.clone()


@pytest.mark.parametrize("between", [None, _edit, _rebind], ids=["plain", "edited", "rebound"])
def test_whole_update_matches_the_graphs(device, monkeypatch, between):
    a0, s0 = _run(device, monkeypatch, False, between)
    a1, s1 = _run(device, monkeypatch, True, between)
    assert s0 == s1
    for (k, p0), p1 in zip(a0.ac.named_parameters(), a1.ac.parameters()):
        assert torch.equal(p0, p1), k
        st0, st1 = a0.optimizer.state[p0], a1.optimizer.state[p1]
        assert torch.equal(st0["exp_avg"], st1["exp_avg"]) and torch.equal(st0["exp_avg_sq"], st1["exp_avg_sq"]), k
        assert torch.equal(st0["step"], st1["step"]), k
