"""GPU: FOMAML's captured and replayed meta step (merlin.fomaml: the inner / outer step graphs recorded after
CAPTURE_AFTER eager steps of a shape, the rollout graphs recorded on a key's first call) held to its eager path bit
for bit, and to the serial restatement of tests/fomaml_ref.py, on one shape, on alternating shapes, across a growth
of the library's module-level scratch, with refreshed weights under a recorded rollout, and through both silent
fallbacks.  Tiny shapes (tasks, k_support, k_query): A = (4, 8, 8), B = (8, 16, 16), C = (4, 16, 16); episodes are
truncated after 6 steps so every rollout holds dones and finished episodes."""
import contextlib
import copy

import pytest
import torch

from fomaml_ref import BATCH_KEYS, assert_meta_gradient, record, serial_meta_gradient

pytestmark = pytest.mark.gpu

A, B, C = (4, 8, 8), (8, 16, 16), (4, 16, 16)
LR_INNER = 0.01


def _fomaml(monkeypatch, device, seed, capture_steps=True):
    """A FOMAML object whose weights and draw seed depend on `seed` alone."""
    from merlin import ScenarioCreator
    from merlin import fomaml as F

    sc = ScenarioCreator()
    monkeypatch.setattr(F, "CAPTURE_STEPS", capture_steps)
    torch.manual_seed(seed)
    fm = F.FOMAML(sc, lr_inner=LR_INNER, lr_outer=3e-4, device=device, difficulty="mediumhard",
                  env_kwargs=dict(sc._env_kwargs("mediumhard"), max_steps=6))
    assert fm.capture_steps is capture_steps and fm.rollout_graph is True
    return fm


def _seeds(step, G):
    return [1000 + 37 * step + g for g in range(G)]


def _step(fm, step, shape):
    G, ks, kq = shape
    return fm.meta_train_step(_seeds(step, G), k_support=ks, k_query=kq)


def _assert_bitwise(fa, ra, fb, rb, where):
    """Parameters, .grad, and the four returned values (loss, reward, steps, the last task's stats) of two objects."""
    assert ra[0] == rb[0] and ra[1] == rb[1] and ra[2] == rb[2], (where, ra[:3], rb[:3])
    assert ra[3] == rb[3], (where, ra[3], rb[3])
    assert 0.0 < ra[2] <= 6.0, (where, ra)  # every task's episodes end inside the query rollout (max_steps = 6 < k)
    for (n, p), q in zip(fa.meta_policy.named_parameters(), fb.meta_policy.parameters()):
        assert torch.equal(p, q), (where, n, (p - q).abs().max().item())
        assert p.grad is not None and q.grad is not None, (where, n)
        assert torch.equal(p.grad, q.grad), (where, n, (p.grad - q.grad).abs().max().item())


def _garbage_grads(fm):
    """Stale .grad tensors a step must not read: new objects, full of NaN."""
    junk = [torch.full_like(p, float("nan")) for p in fm.meta_policy.parameters()]
    for p, j in zip(fm.meta_policy.parameters(), junk):
        p.grad = j
    return junk


def _assert_fresh(fm, junk, where):
    for (n, p), j in zip(fm.meta_policy.named_parameters(), junk):
        assert p.grad is not j and bool(torch.isfinite(p.grad).all()), (where, n)


def test_two_eager_objects_are_bitwise_equal(monkeypatch, device):
    """The precondition of every bitwise claim below: the eager meta step (rollout graphs on, step graphs off) is
    reproducible bit for bit -- two objects of one seed, 5 steps of shape A, equal after every step.  One of them is
    handed NaN-filled .grad tensors before two of its steps: an eager step reads no stale gradient."""
    fa = _fomaml(monkeypatch, device, 5, capture_steps=False)
    fb = _fomaml(monkeypatch, device, 5, capture_steps=False)
    assert fa._act_seed == fb._act_seed
    for step in range(5):
        junk = _garbage_grads(fb) if step in (1, 3) else None
        ra, rb = _step(fa, step, A), _step(fb, step, A)
        _assert_bitwise(fa, ra, fb, rb, (step, A))
        if junk is not None:
            _assert_fresh(fb, junk, step)
    for fm in (fa, fb):
        assert fm.capture_steps is False and "inner" not in fm._steps[A] and fm._steps[A]["eager"] == 5
        assert int(fm._act_epoch.item()) == 2 * (5 + 1)  # two rollouts per step, one more draw at each recording


def test_captured_and_replayed_steps_equal_eager_steps(monkeypatch, device):
    """CAPTURE_AFTER + 3 steps of shape A on a capturing object and on an eager-step control: equal bit for bit after
    every step -- the two eager steps, the capture step (whose result is the graphs' first replay) and two replays.
    On the replayed steps .grad is the captured tensor, also after a stale tensor was put there."""
    from merlin import fomaml as F

    fc = _fomaml(monkeypatch, device, 6, capture_steps=True)
    fe = _fomaml(monkeypatch, device, 6, capture_steps=False)
    n_steps = F.CAPTURE_AFTER + 3
    for step in range(n_steps):
        junk_e = _garbage_grads(fe) if step in (1, F.CAPTURE_AFTER + 1) else None
        junk_c = _garbage_grads(fc) if step == n_steps - 1 else None  # a replay reads the captured tensors, not .grad
        rc, re_ = _step(fc, step, A), _step(fe, step, A)
        _assert_bitwise(fc, rc, fe, re_, (step, A))
        assert int(fc._act_epoch.item()) == int(fe._act_epoch.item())
        if junk_e is not None:
            _assert_fresh(fe, junk_e, step)
        if junk_c is not None:
            _assert_fresh(fc, junk_c, step)
        st = fc._steps[A]
        if step >= F.CAPTURE_AFTER:
            assert st.get("inner") is not None and st.get("outer") is not None, step
            assert len(st["grads"]) == len(list(fc.meta_policy.parameters()))
            for p, g in zip(fc.meta_policy.parameters(), st["grads"]):
                assert p.grad is g, step
        else:
            assert "inner" not in st and "outer" not in st and st["eager"] == step + 1
    assert fc.capture_steps is True and fc.rollout_graph is True
    assert fe.capture_steps is False and "inner" not in fe._steps[A]


def test_replayed_step_matches_serial_reference(monkeypatch, device):
    """The capture step and the replay after it against the serial restatement on the recorded batches: the average
    query loss and every parameter's clipped meta gradient, at the eager test's bounds.
    Measured: the capture step 4.3e-5 of the scale, the replay 2.6e-5, both critic.2.bias (a factor of 2.3 under the
    bound, at the serial side's own noise: fomaml_ref.assert_meta_gradient); every other tensor under 2e-6."""
    from merlin import fomaml as F

    fm = _fomaml(monkeypatch, device, 7)
    recorded = []
    record(fm, recorded)
    for step in range(F.CAPTURE_AFTER + 2):
        meta0 = copy.deepcopy(fm.meta_policy)
        del recorded[:]
        ret = _step(fm, step, A)
        if step < F.CAPTURE_AFTER:
            continue
        assert fm._steps[A].get("outer") is not None
        support, query = recorded
        assert support["rew"].shape == (A[1], A[0]) and bool((query["done"] > 0).any())
        meta, qlosses, gnorm = serial_meta_gradient(meta0, support, query, LR_INNER)
        assert_meta_gradient(fm, ret[0], meta, qlosses, gnorm)


def test_alternating_shapes(monkeypatch, device):
    """A, B (other task count: the env is replaced, the scratch grows), A, C (other k: the env stays), A -- each past
    its capture -- on a capturing object and an eager-step control: equal bit for bit after every step.  And, with no
    luck needed from the allocator: a step graph is only ever replayed with the rollout storage tensors it was
    captured with, and a rollout graph only on the env it was recorded on, which is the live one."""
    from merlin import fomaml as F

    fc = _fomaml(monkeypatch, device, 8, capture_steps=True)
    fe = _fomaml(monkeypatch, device, 8, capture_steps=False)
    seen = {}
    orig = fc.collect_trajectory

    def watch(env, params, steps, key="rollout", **kw):
        b = orig(env, params, steps, key=key, **kw)
        seen[key] = (tuple(b[k] for k in BATCH_KEYS), fc._rollouts[key]["graph"], env)
        return b

    fc.collect_trajectory = watch
    ca = F.CAPTURE_AFTER
    schedule = [A] * (ca + 2) + [B] * (ca + 2) + [A] * 2 + [C] * (ca + 1) + [A]
    step_bound, rollout_bound = {}, {}  # id(graph) -> (graph, the tensors it ran with first[, its env])
    replays = 0
    for step, shape in enumerate(schedule):
        before = {n: fc._steps.get(shape, {}).get(n) for n in ("inner", "outer")}
        rc, re_ = _step(fc, step, shape), _step(fe, step, shape)
        _assert_bitwise(fc, rc, fe, re_, (step, shape))
        for name, kind in (("inner", "support"), ("outer", "query")):
            tensors, rgraph, env = seen[kind]
            assert env is fc._env and env.num_envs == shape[0], (step, shape)
            assert rgraph is not None, (step, kind)
            first = rollout_bound.setdefault(id(rgraph), (rgraph, tensors, env))
            assert first[2] is env, (step, shape, kind, "a rollout graph replayed on another env than it recorded")
            assert all(x is y for x, y in zip(first[1], tensors)), (step, shape, kind)
            g = fc._steps[shape].get(name)
            if g is None:
                continue
            replays += before[name] is g
            first = step_bound.setdefault(id(g), (g, tensors))
            assert all(x is y for x, y in zip(first[1], tensors)), \
                (step, shape, name, "a step graph replayed with other storage than it captured")
    # A and B were replayed from graphs of an earlier step, A at once on each return (its graphs are kept, not
    # recorded again): inner + outer at one step of A, one of B, two of A, one of A
    assert replays == 2 * (1 + 1 + 2 + 1)
    assert fc.capture_steps is True and fc.rollout_graph is True and fe.rollout_graph is True
    for shape in (A, B, C):
        assert fc._steps[shape].get("inner") is not None and fc._steps[shape].get("outer") is not None


def test_scratch_growth_under_a_live_capture(monkeypatch, device):
    """The grouped histogram's slab scratch is one module-level buffer per device, replaced when a call needs more.
    Shape A's step graphs recorded the small one: after a plain eager evaluate + backward at a larger (G, F) has
    replaced it, the graphs' owner still holds the recorded buffer where it was, memory allocated since is not
    written by the replays, and two more steps of A equal the control's."""
    from merlin import _native as nat
    from merlin import fomaml as F
    from merlin import grouped_policy as gp
    from test_gpu_grouped_policy import _codes, _tasks

    monkeypatch.setattr(nat, "_SLABS", {})  # whatever earlier tests left: A allocates its own, small
    fc = _fomaml(monkeypatch, device, 9, capture_steps=True)
    fe = _fomaml(monkeypatch, device, 9, capture_steps=False)
    step = 0
    for step in range(F.CAPTURE_AFTER + 1):
        _assert_bitwise(fc, _step(fc, step, A), fe, _step(fe, step, A), (step, A))
    st = fc._steps[A]
    small = nat._SLABS[device]
    need_a = int(nat.lib().merlin_tower_conv2_lut_slab_bytes(2 * A[0], A[1]))
    assert small.numel() == need_a
    held = {name: st[name + "_bound"] for name in ("inner", "outer")}
    for name, bound in held.items():
        assert len(bound) == 1 and bound[0] is small, name
    ptr = small.data_ptr()
    del small
    G2, F2 = 8, 300  # 16 towers, two frame blocks per tower: four times A's slabs
    assert int(nat.lib().merlin_tower_conv2_lut_slab_bytes(2 * G2, F2)) >= 4 * need_a
    _, params = _tasks(device, G2, seed=3)
    codes = _codes(device, G2 * F2, seed=5)
    acts = torch.randint(0, 3, (G2, F2), device=device)
    for _ in range(2):  # once next to each object
        lp, ent, v = gp.evaluate(params, codes, F2, acts)
        (lp.sum() + v.sum() + ent.sum()).backward()
    assert nat._SLABS[device].numel() >= 4 * need_a and nat._SLABS[device].data_ptr() != ptr
    for name, bound in held.items():
        assert st[name + "_bound"] is bound and len(bound) == 1 and bound[0].data_ptr() == ptr, name
        assert bound[0].numel() == need_a
    # a block of the recorded buffer's size allocated now: the recorded buffer is still allocated, so this is other
    # memory and no replay writes it
    canary = torch.full((need_a,), 0x5A, dtype=torch.uint8, device=device)
    assert canary.data_ptr() != ptr
    for step in range(F.CAPTURE_AFTER + 1, F.CAPTURE_AFTER + 3):
        _assert_bitwise(fc, _step(fc, step, A), fe, _step(fe, step, A), (step, A))
    assert bool((canary == 0x5A).all())
    assert fc.capture_steps is True and st["inner_bound"][0].data_ptr() == ptr


def _per_task_models(meta_policy, params, G):
    models = []
    for g in range(G):
        m = copy.deepcopy(meta_policy)
        with torch.no_grad():
            for n, p in m.named_parameters():
                p.copy_(params[n][g])
        models.append(m)
    return models


def _worst(got, ref):
    """max |got - ref| / (atol + rtol |ref|) at rtol = atol = 1e-5: <= 1 is torch.testing.assert_close's pass."""
    return ((got - ref).abs() / (1e-5 + 1e-5 * ref.abs())).max().item()


def test_replayed_rollouts_act_with_the_refreshed_weights(monkeypatch, device):
    """Three rollouts on one key with three per-task weight stacks: the first records the graph, the others replay it
    after the in-place refresh.  Every returned logp / value / bootstrap value is what each task's own weights OF
    THAT CALL give on the recorded frames and actions (per-task CNNActorCritic.evaluate_codes, rtol = atol = 1e-5),
    and is far from what the previous call's weights give.  Then: the same rollouts, bit for bit, from an object that
    launches them eagerly at the same draw epochs."""
    from merlin import batched_policy as bp

    G, k = 4, 8
    fm = _fomaml(monkeypatch, device, 10)
    fe = _fomaml(monkeypatch, device, 10)
    fe.rollout_graph = False
    seeds = _seeds(0, G)
    env, env_e = fm._task_env(seeds), fe._task_env(seeds)
    gen = torch.Generator(device=device)
    gen.manual_seed(11)
    meta = {n: p.detach() for n, p in bp.stack_params(fm.meta_policy, G).items()}

    def perturbed():  # distinct weights per task, all within the init's scale
        return {n: p + torch.randn(p.shape, device=device, generator=gen) * 0.05 * (p.abs().mean() + 1e-3)
                for n, p in meta.items()}

    stacks = [meta, perturbed(), perturbed()]
    graph = None
    for call, params in enumerate(stacks):
        b = fm.collect_trajectory(env, params, k, key="probe")
        got = {key: b[key].clone() for key in BATCH_KEYS}
        epoch = int(fm._act_epoch.item())  # the epoch the returned rollout drew with
        assert epoch == (2 if call == 0 else call + 2)
        st = fm._rollouts["probe"]
        assert st["graph"] is not None and (graph is None or st["graph"] is graph)  # recorded once, then replayed
        graph = st["graph"]
        assert bool((got["done"] > 0).any()) and len(b["ep_lens"]) == int((got["done"] > 0).sum())

        def errors(weights):
            worst = 0.0
            for g, m in enumerate(_per_task_models(fm.meta_policy, weights, G)):
                with torch.no_grad():
                    lp, _, v = m.evaluate_codes(got["codes"][:k, g].contiguous(), got["act"][:, g])
                    _, _, vl = m.evaluate_codes(got["codes"][k:, g].contiguous(), got["act"][:1, g])
                worst = max(worst, _worst(got["logp"][:, g], lp), _worst(got["val"][:, g], v),
                            _worst(got["last_val"][g:g + 1], vl))
            return worst

        own = errors(params)
        print(f"call {call}: worst error / tolerance with the call's own weights {own:.3g}", end="")
        assert own <= 1.0, (call, own)
        if call:
            stale = errors(stacks[call - 1])
            print(f", with the previous call's {stale:.3g}", end="")
            # a 5 % change of every weight moves values of order 0.1 - 1 by some 1e-3 - 1e-2, against 1e-5: a pass
            # on stale weights would need an error 10 times under what the perturbation causes at the very least
            assert stale > 10.0, (call, stale)
        print()
        # the eager twin, its counter set so that its (single) bump lands on the same epoch
        fe._act_epoch.fill_(epoch - 1)
        be = fe.collect_trajectory(env_e, params, k, key="probe")
        assert fe._rollouts["probe"]["graph"] is None and int(fe._act_epoch.item()) == epoch
        for key in BATCH_KEYS:
            assert torch.equal(got[key], be[key]), (call, key)


def _refusing_guard(monkeypatch, flag):
    """merlin._native.capture_guard raising on entry while flag["on"]: before torch.cuda.graph is entered, so no
    capture is open when it fires."""
    from merlin import _native as nat

    real = nat.capture_guard

    @contextlib.contextmanager
    def guard():
        if flag["on"]:
            raise RuntimeError("capture refused (test)")
        with real() as bound:
            yield bound

    monkeypatch.setattr(nat, "capture_guard", guard)


def test_step_capture_fallback_equals_eager(monkeypatch, device):
    """The step capture refused at the third step: that step falls back to eager launches, capture_steps goes off,
    no graph is stored, and this step and two more equal the eager control's bit for bit."""
    from merlin import fomaml as F

    flag = {"on": False}
    _refusing_guard(monkeypatch, flag)
    fc = _fomaml(monkeypatch, device, 12, capture_steps=True)
    fe = _fomaml(monkeypatch, device, 12, capture_steps=False)
    for step in range(F.CAPTURE_AFTER + 3):
        flag["on"] = step >= F.CAPTURE_AFTER
        _assert_bitwise(fc, _step(fc, step, A), fe, _step(fe, step, A), (step, A))
        assert fc.capture_steps is (step < F.CAPTURE_AFTER)
    st = fc._steps[A]
    assert "inner" not in st and "outer" not in st and "grads" not in st
    assert fc.rollout_graph is True and fc._rollouts["support"]["graph"] is not None  # recorded before the refusal


def test_rollout_capture_fallback_matches_serial_reference(monkeypatch, device):
    """Every capture refused from the start: the rollouts stay eager (rollout_graph off, no graph stored), so do the
    steps, and each step still passes the serial-reference check.  (Its draws are keyed by other epochs than a
    recording object's: nothing bitwise to compare with.)
    The serial side has outliers of its own at these bounds (fomaml_ref.assert_meta_gradient), about one step in
    thirty, on eager steps like any other: with seed 13 this test's first step gave critic.2.bias 1.56e-4 of its scale,
    with seed 7 its third step met a ReLU tie (one of critic.0.bias's 512 entries, 2.7e-2 of the tensor's scale).  Seeds
    1 .. 8 were measured with every capture refused; 1 is the first whose three steps are all clear of the bounds by a
    factor of 2 (worst: critic.2.bias 2.1e-5, every other tensor 1.1e-6)."""
    from merlin import fomaml as F

    flag = {"on": True}
    _refusing_guard(monkeypatch, flag)
    fm = _fomaml(monkeypatch, device, 1, capture_steps=True)
    recorded = []
    record(fm, recorded)
    for step in range(F.CAPTURE_AFTER + 1):
        meta0 = copy.deepcopy(fm.meta_policy)
        del recorded[:]
        ret = _step(fm, step, A)
        assert fm.rollout_graph is False
        assert fm._rollouts["support"]["graph"] is None and fm._rollouts["query"]["graph"] is None
        assert int(fm._act_epoch.item()) == 2 * (step + 1)  # one draw per rollout: nothing was replayed
        support, query = recorded
        meta, qlosses, gnorm = serial_meta_gradient(meta0, support, query, LR_INNER)
        assert_meta_gradient(fm, ret[0], meta, qlosses, gnorm)
    assert fm.capture_steps is False and "inner" not in fm._steps[A] and "outer" not in fm._steps[A]
