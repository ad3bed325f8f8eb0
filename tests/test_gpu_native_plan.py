"""GPU: the native planner (csrc/merlin_plan.hip, windows.NATIVE_PLAN) against the torch builders it replaces, array
for array with equal dtypes, shapes and elements.  Phase 1, WindowPlan.native against FrameGroups + WindowPlan: uid,
wid, rows, kid, the counts and every SegmentPlan's key / idx / fix / head_fix / item_len / nitems; rep by its defining
property (a member of its group).  Phase 2, update_minibatches(bulk=True) with the switch on against off: groups,
inv, slot, order, offs, kmap; rep_row by its defining property (a row of the minibatch holding the same patch).
Synthetic observations drawn from a pool of random 7x7 class grids, no env; then one PPO update with the switch on
and one with it off: bitwise equal parameters and statistics."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ARRAYS = ("groups", "inv", "slot", "order", "offs", "kmap")


def _codes(device, B, pool, seed, sparse=False):
    """int32 [B, 8] observation codes: B draws from `pool` random class grids (cell r*7 + c = nibble cell % 8 of
    word cell // 8), every pool entry used at least once when B >= pool.  sparse: nine cells in ten are class 0, so
    distinct frames share windows, patches and bands (long runs in every list)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    cls = torch.randint(0, 5, (pool, 64), generator=g)
    if sparse:
        cls = cls * (torch.rand((pool, 64), generator=g) < 0.1)
    cls[:, 49:] = 0
    words = (cls.view(pool, 8, 8) << (4 * torch.arange(8))).sum(2)  # < 2^31: classes are below 8
    pick = torch.cat([torch.arange(min(pool, B)), torch.randint(0, pool, (max(0, B - pool),), generator=g)])
    pick = pick[torch.randperm(B, generator=g)]
    return words[pick].to(torch.int32).to(device).contiguous()


def _plan(device, B, pool, seed=0):
    from merlin.dedup import FrameGroups
    from merlin.windows import WindowPlan

    codes = _codes(device, B, pool, seed)
    fg = FrameGroups(codes)
    assert fg.ok and fg.num_groups <= pool
    return WindowPlan(codes, fg)


def _perms(device, B, epochs, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return [torch.randperm(B, device=device, generator=g) for _ in range(epochs)]


def _both(monkeypatch, plan, perms, mbs):
    from merlin import windows as W

    monkeypatch.setattr(W, "NATIVE_PLAN", False)
    ref = plan.update_minibatches(perms, mbs, bulk=True)
    monkeypatch.setattr(W, "NATIVE_PLAN", True)
    got = plan.update_minibatches(perms, mbs, bulk=True)
    assert type(got[0][0]).__name__ == "_BulkViews"  # the native builder ran
    return ref, got


def _assert_same(plan, ref, got):
    assert len(ref) == len(got)
    for er, eg in zip(ref, got):
        assert len(er) == len(eg)
        for r, g in zip(er, eg):
            for name in ARRAYS:
                a, b = getattr(r, name), getattr(g, name)
                assert a.dtype == b.dtype and a.shape == b.shape, name
                assert torch.equal(a, b), name
            n = int(g.groups.numel())
            rr = g.rep_row.long()
            assert g.rep_row.dtype == torch.int32 and rr.numel() == n * 9
            assert bool((rr >= 0).all()) and bool((rr < n * 9).all())
            live = plan.kid[g.groups].reshape(-1)
            assert torch.equal(live[rr], live)  # the representative holds the row's patch
            assert torch.equal(rr[rr], rr)  # and represents itself
            assert int((rr == torch.arange(n * 9, device=rr.device)).sum()) == int((g.kmap >= 0).sum())


@pytest.mark.parametrize("pool", [1, 37, 2048])
def test_minibatch_arrays_match_torch(device, monkeypatch, pool):
    """B = 2,048: one frame, many repeats, all distinct; 3 epochs x 4 minibatches of 512."""
    plan = _plan(device, 2048, pool)
    ref, got = _both(monkeypatch, plan, _perms(device, 2048, 3, 1), 512)
    _assert_same(plan, ref, got)


def test_ragged_last_minibatch(device, monkeypatch):
    """B = 2,000 in 3 epochs x minibatches of 768: the last of each epoch holds 464 samples."""
    plan = _plan(device, 2000, 300)
    ref, got = _both(monkeypatch, plan, _perms(device, 2000, 3, 2), 768)
    assert [int(m.inv.numel()) for m in got[0]] == [768, 768, 464]
    _assert_same(plan, ref, got)


def test_workspace_reuse_and_growth(device, monkeypatch):
    """A second and a third call on the same workspace with a smaller B, then a larger one: stale scratch from the
    call before must not show, and the workspace grows."""
    from merlin import windows as W

    monkeypatch.setattr(W, "_PLAN_WORKSPACE", W.nat.PlanWorkspace())
    sizes = []
    for B, pool, mbs in ((2048, 200, 512), (640, 50, 256), (5000, 900, 1024)):
        plan = _plan(device, B, pool, seed=B)
        ref, got = _both(monkeypatch, plan, _perms(device, B, 2, B), mbs)
        _assert_same(plan, ref, got)
        sizes.append(int(W._PLAN_WORKSPACE.buf.numel()))
    assert sizes[1] == sizes[0] and sizes[2] > sizes[1]


def test_two_calls_same_bits(device, monkeypatch):
    plan = _plan(device, 2048, 37)
    perms = _perms(device, 2048, 3, 4)
    _, a = _both(monkeypatch, plan, perms, 512)
    b = plan.update_minibatches(perms, 512, bulk=True)
    for ea, eb in zip(a, b):
        for x, y in zip(ea, eb):
            for name in ARRAYS + ("rep_row",):
                assert torch.equal(getattr(x, name), getattr(y, name)), name


def test_out_of_range_index_is_reported(device, monkeypatch):
    """An index past the rollout raises after the host read (taken as frame 0 inside: nothing indexes out of
    bounds)."""
    from merlin import _native as nat
    from merlin import windows as W

    plan = _plan(device, 2048, 37)
    perms = _perms(device, 2048, 1, 5)
    perms[0][7] = 2048
    monkeypatch.setattr(W, "NATIVE_PLAN", True)
    with pytest.raises(nat.MerlinNativeError):
        plan.update_minibatches(perms, 512, bulk=True)


LISTS = ("hist", "patch_plan", "band_plan", "dq_plan")


def _assert_same_plan(codes, ref, got):
    """WindowPlan `got` (native) against `ref` (torch) and their frame groups."""
    fr, fg = ref.frame_groups, got.frame_groups
    assert fg.ok and fr.ok and fg.num_groups == fr.num_groups
    assert fg.uid.dtype == fr.uid.dtype and torch.equal(fg.uid, fr.uid)
    assert fg.rep.dtype == fr.rep.dtype and fg.rep.shape == fr.rep.shape
    assert torch.equal(fg.uid[fg.rep], torch.arange(fg.num_groups, device=codes.device))  # a member of its group
    assert torch.equal(codes[fg.rep[fg.uid]], codes)
    for name in ("num_frames", "num_windows", "num_patches", "num_bands"):
        assert getattr(got, name) == getattr(ref, name), name
    for name in ("wid", "rows", "kid"):
        a, b = getattr(ref, name), getattr(got, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    for lst in LISTS:
        a, b = getattr(ref, lst), getattr(got, lst)
        assert (a.nnz, a.item_len, a.nitems) == (b.nnz, b.item_len, b.nitems), lst
        for name in ("key", "idx", "fix", "head_fix", "counters"):
            x, y = getattr(a, name), getattr(b, name)
            assert x.dtype == y.dtype and x.shape == y.shape and y.is_contiguous(), (lst, name)
            assert torch.equal(x, y), (lst, name)


def _plans(device, B, pool, seed=0, sparse=False, **item):
    from merlin.dedup import FrameGroups
    from merlin.windows import WindowPlan

    codes = _codes(device, B, pool, seed, sparse)
    ref = WindowPlan(codes, FrameGroups(codes), **item)
    fg, got = WindowPlan.native(codes, **item)
    assert got is not None and got.frame_groups is fg
    c = got.native_counts.tolist()
    assert c[:7] == [got.num_frames, 0, got.num_windows, 0, got.num_patches, got.num_bands, 0]
    return codes, ref, got


@pytest.mark.parametrize("pool", [1, 37, 2048])
def test_plan_arrays_match_torch(device, pool):
    """B = 2,048: one frame, many repeats, all distinct; the lists cut by auto_item_len."""
    _assert_same_plan(*_plans(device, 2048, pool))


@pytest.mark.parametrize("B,pool", [(2048, 37), (2000, 2000)])
def test_plan_lists_cross_items(device, B, pool):
    """item_len = 32 on every list: destinations start in one item and end in a later one (live fix rows, head
    fixes) at these sizes."""
    codes, ref, got = _plans(device, B, pool, seed=3, sparse=True, item_len=32, hist_item_len=32)
    for lst in LISTS:
        sp = getattr(ref, lst)
        assert sp.nitems > 1, lst
        assert bool((sp.fix[:, 0] >= 0).any()) and bool((sp.head_fix >= 0).any()), lst
    _assert_same_plan(codes, ref, got)


def test_plan_workspace_reuse_and_same_bits(device, monkeypatch):
    """The same workspace for a smaller, then a larger rollout, and the same call twice: equal arrays."""
    from merlin import windows as W

    monkeypatch.setattr(W, "_PLAN_WORKSPACE", W.nat.PlanWorkspace())
    for B, pool in ((2048, 300), (640, 50), (5000, 1200)):
        codes, ref, got = _plans(device, B, pool, seed=B, item_len=32)
        _assert_same_plan(codes, ref, got)
        _, again = W.WindowPlan.native(codes, item_len=32)
        _assert_same_plan(codes, got, again)
        assert torch.equal(again.frame_groups.rep, got.frame_groups.rep)


def test_native_plan_feeds_native_minibatches(device, monkeypatch):
    """The native plan under the native minibatch builder == the torch plan under the torch builder."""
    from merlin import windows as W

    codes, ref, got = _plans(device, 2000, 300, seed=9)
    perms = _perms(device, 2000, 3, 6)
    monkeypatch.setattr(W, "NATIVE_PLAN", False)
    a = ref.update_minibatches(perms, 768, bulk=True)
    monkeypatch.setattr(W, "NATIVE_PLAN", True)
    b = got.update_minibatches(perms, 768, bulk=True)
    _assert_same(got, a, b)


def test_colliding_hashes_fall_back(device, monkeypatch):
    """All-zero multipliers: every hash is 0, one group holds different frames, ok is False (as the torch groups
    say) and no plan is built; the update then evaluates every sample, with the switch on as with it off."""
    from merlin import dedup
    from merlin.windows import WindowPlan

    monkeypatch.setattr(dedup, "_MULT", (0,) * 8)
    codes = _codes(device, 2048, 37, 1)
    assert not dedup.FrameGroups(codes).ok
    fg, plan = WindowPlan.native(codes)
    assert not fg.ok and plan is None and fg.num_groups == 1
    _, s0 = _update(device, False, monkeypatch, fast=False)
    _, s1 = _update(device, True, monkeypatch, fast=False)
    assert s0 == s1


def _update(device, native, monkeypatch, fast=True):
    from merlin import MerlinVecEnv
    from merlin import windows as W
    from merlin.ppo import PPO

    monkeypatch.setattr(W, "NATIVE_PLAN", native)
    env = MerlinVecEnv(64, "mediumhard", seed=5, device=device)
    torch.manual_seed(3)
    agent = PPO(env, lr=1e-3, batch_size=64 * 32, minibatch_size=64 * 8, update_epochs=2, ent_coef=0.05,
                device=device)
    stats = agent.update(agent.collect_rollouts())
    torch.cuda.synchronize()
    assert (agent._wstep is not None) == fast  # the bulk path, unless the groups were not ok
    return agent, stats


def test_ppo_update_bitwise_equal(device, monkeypatch):
    """One PPO update on 64 envs x 32 steps with the switch on and one with it off."""
    a0, s0 = _update(device, False, monkeypatch)
    a1, s1 = _update(device, True, monkeypatch)
    assert s0 == s1
    for (k, p0), p1 in zip(a0.ac.named_parameters(), a1.ac.parameters()):
        assert torch.equal(p0, p1), k
