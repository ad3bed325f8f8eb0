"""GPU: level editing.

Kernel    merlin_levels_mutate equals merlin_levels_mutate_host bit for bit (the host entry is held to the numpy
          reference by tests/test_level_edit_host.py): C in {1, 2, 3, 8, 9, 257} (the odd half wave, the 8-per-block
          seam, many blocks), the five sizes, E in {0, 1, 16}; dist equals merlin_shortest_paths on the children;
          out-of-range parents leave zeros; canary words around every output buffer are intact.
Bank      merlin_env_replace_levels with N = 64, L = 8, S = 7: exactly the replaced slots change, slots -1 and L are
          skipped; a reset under a CDF concentrated on a replaced slot plays the child; an env in the middle of an
          episode in a replaced slot keeps its walls, logs -1, draws its next map as before; a captured multi-step graph
          plays the new map without a re-capture.
Trainer   PPO(level_editor=...): the env's bank equals the trainer's set after every iteration, replaced slots are
          unseen, lineage is consistent, the graph and the eager run build the same banks, one capture.
"""
import numpy as np
import pytest
import torch

import level_edit_ref as R
import level_ref as LR

pytestmark = pytest.mark.gpu

GUARD = 16
CANARY = 0x5A5A5A5A
COUNTS = (1, 2, 3, 8, 9, 257)


def parent_index(C):
    """Parents 0 and 1 of a two-map bank, with entries outside it: 2, -1 and large ones."""
    p = (np.arange(C, dtype=np.int64) * 7) % 3
    p[np.arange(C) % 11 == 5] = -1
    p[np.arange(C) % 13 == 7] = 1 << 30
    p[np.arange(C) % 17 == 9] = -(1 << 31)
    return p.astype(np.int32)


def guarded(C, S, device):
    """The five outputs as views into two canary-filled buffers, with GUARD words (bytes for `changed`) around each."""
    sizes = [C * S, C * 2, C * 4, C]
    buf = torch.full((GUARD + sum(n + GUARD for n in sizes),), CANARY, dtype=torch.int32, device=device)
    views, inside, at = [], torch.zeros(buf.numel(), dtype=torch.bool), GUARD
    for n, shape in zip(sizes, [(C, S), (C, 2), (C, 4), (C,)]):
        views.append(buf[at:at + n].view(shape))
        inside[at:at + n] = True
        at += n + GUARD
    cb = torch.full((GUARD + C + GUARD,), 0x5A, dtype=torch.uint8, device=device)
    views.append(cb[GUARD:GUARD + C])
    return views, buf, inside, cb


@pytest.mark.parametrize("S", R.SIZES)
@pytest.mark.parametrize("E", [0, 1, 16])
def test_kernel_equals_host(device, S, E):
    from merlin import _native as nat

    walls, goal, agent = R.bank([R.serpentine(S), R.open_room(S)])
    dw, dg, da = (torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
                  for a in (walls, goal, agent))
    for C in COUNTS:
        pidx = parent_index(C)
        ref = nat.levels_mutate_host(walls, goal, agent, pidx, S, E, R.EDIT_SEED, R.GENERATION)
        views, buf, inside, cb = guarded(C, S, device)
        got = nat.levels_mutate(dw, dg, da, torch.from_numpy(pidx).to(device), S, E, R.EDIT_SEED, R.GENERATION,
                                out=tuple(views))
        torch.cuda.synchronize(device)
        for name, g, r in zip(("walls", "goal", "agent", "dist", "changed"), got, ref):
            g = g.cpu().numpy()
            assert (g.view(r.dtype) == r).all(), (name, C)
        assert (buf.cpu()[~inside] == CANARY).all(), C
        cbh = cb.cpu()
        assert (cbh[:GUARD] == 0x5A).all() and (cbh[GUARD + C:] == 0x5A).all(), C
        # dist is merlin_shortest_paths' on the children; a parent outside the bank leaves zeros, dist -1, changed 0
        ok = (pidx >= 0) & (pidx < 2)
        kw, kg, ka, dist, changed = (t.contiguous() for t in got)
        sp = nat.shortest_paths(kw, kg, ka, S).cpu().numpy()
        assert (sp[ok] == ref[3][ok]).all(), C
        if (~ok).any():
            bad = torch.from_numpy(~ok).to(device)
            assert not kw[bad].any() and not kg[bad].any() and not ka[bad].any()
            assert (dist[bad] == -1).all() and not changed[bad].any()
        if E == 0:
            assert not changed.any()
    if S in (5, 7) and E == 1:  # the inputs reach the branches: unchanged, unsolvable and changed children among 257
        assert (ref[4][ok] == 0).any() and (ref[3][ok] < 0).any() and ((ref[4] == 1) & (ref[3] > 0)).any()


def test_kernel_null_parent_index_and_key(device):
    from merlin import _native as nat

    S, E = 16, 4
    walls, goal, agent = R.bank([R.serpentine(S), R.open_room(S)] * 5)
    dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device) for a in (walls, goal, agent)]
    for count in (10, 3):
        ref = nat.levels_mutate_host(walls, goal, agent, None, S, E, (1 << 64) - 1, (1 << 63) + 5, count=count)
        got = nat.levels_mutate(*dev, None, S, E, (1 << 64) - 1, (1 << 63) + 5, count=count)
        for g, r in zip(got, ref):
            assert g.shape[0] == count and (g.cpu().numpy().view(r.dtype) == r).all()
    with pytest.raises(nat.MerlinNativeError) as e:
        nat.levels_mutate(*dev, None, S, E, 1, 1, count=11)  # NULL index: C <= P
    assert e.value.code == nat.E_INVALID


# ------------------------------------------------------------------------------------------------------------- bank
N, L, S7 = 64, 8, 7
LEVEL_SEED = 7
UNIFORM = np.arange(1, L + 1, dtype=np.float64) / L
_MAPS = {}


def maps():
    """(bank, kids): 8 + 6 distinct solvable 7x7 levels, children of the serpentine under the reference."""
    if not _MAPS:
        ow, og, oa, dist, changed, _ = R.outcome(R.serpentine, S7, 4)
        keep, seen = [], set()
        for c in np.flatnonzero((dist > 0) & (changed == 1)):
            key = ow[c].tobytes() + og[c].tobytes() + oa[c].tobytes()
            if key not in seen:
                seen.add(key)
                keep.append(c)
        assert len(keep) >= L + 6
        pick = lambda idx: tuple(np.ascontiguousarray(a[idx]) for a in (ow.view(np.int32), og, oa))  # noqa: E731
        _MAPS["bank"], _MAPS["kids"] = pick(keep[:L]), pick(keep[L:L + 6])
    return _MAPS["bank"], _MAPS["kids"]


def make_env(device, max_steps=50, bind=True):
    from merlin import MerlinVecEnv
    from merlin.levels import LevelSet

    env = MerlinVecEnv(N, difficulty="easy", size=S7, seed=31, device=device, max_steps=max_steps)
    if bind:
        env.set_levels(LevelSet.from_arrays(*maps()[0], device=device), LEVEL_SEED)
    return env


def dev_kids(device, idx):
    return tuple(torch.from_numpy(np.ascontiguousarray(a[idx])).to(device) for a in maps()[1])


def i32(device, v):
    return torch.tensor(v, dtype=torch.int32, device=device)


def bank_np(env):
    return tuple(t.cpu().numpy() for t in env.level_bank())


def test_level_bank_and_replaced_slots(device):
    bank, kids = maps()
    env = make_env(device)
    for got, want in zip(bank_np(env), bank):
        assert (got == want).all()
    env.replace_levels(i32(device, [3, -1, L, 0, -(1 << 31), 1 << 30]), dev_kids(device, slice(0, 6)))
    want = [a.copy() for a in bank]
    for a, k in zip(want, kids):
        a[3], a[0] = k[0], k[3]
    for got, w in zip(bank_np(env), want):
        assert (got == w).all()
    # a CDF concentrated on a replaced slot: a reset makes every env's snapshot the child
    env.set_level_cdf(torch.from_numpy(LR.cdf_of(np.eye(L)[3])).to(device))
    env.reset()
    walls, goal, agent = (t.cpu().numpy() for t in env.snapshot())
    assert (walls == kids[0][0]).all() and (goal == kids[1][0]).all() and (agent == kids[2][0]).all()
    assert (env.current_levels() == 3).all()
    env.errors()
    env.close()


def test_replace_needs_a_bound_bank(device):
    from merlin import _native as nat

    env = make_env(device, bind=False)
    with pytest.raises(nat.MerlinNativeError) as e:
        env.replace_levels(i32(device, [0]), dev_kids(device, slice(0, 1)))
    assert e.value.code == nat.E_INVALID
    with pytest.raises(nat.MerlinNativeError) as e:
        env.level_bank()
    assert e.value.code == nat.E_INVALID
    env.close()


def test_env_inside_a_replaced_slot(device):
    """max_steps 6, turns only (no episode ends early): two steps, slot s replaced, four steps to the truncation, two
    more.  Against a twin env that is stepped alike with nothing replaced."""
    from merlin import _native as nat

    bank, kids = maps()
    T, cut = 8, 2
    envs = [make_env(device, max_steps=6) for _ in range(2)]
    logs = [torch.full((T, N), -7, dtype=torch.int32, device=device) for _ in range(2)]
    acts = torch.zeros(N, dtype=torch.int64, device=device)
    done = torch.zeros((T, N), dtype=torch.float32, device=device)
    for env in envs:
        env.reset()
    first = envs[0].current_levels().cpu().numpy()
    assert (first == LR.draws(LEVEL_SEED, 0, N, 0, 1, UNIFORM)[:, 0]).all()
    s = int(first[0])
    inside = first == s
    assert 0 < inside.sum() < N
    before = []
    for t in range(T):
        if t == cut:
            envs[0].replace_levels(i32(device, [-1, s]), dev_kids(device, slice(0, 2)))
        for env, log in zip(envs, logs):
            env.set_level_log(log[t])
            env.step_into(acts, None, None, None, None, done[t])
        if t == 4:  # still in the first episode: the old map, in both envs
            before = [tuple(x.cpu().numpy() for x in env.snapshot()) for env in envs]
    torch.cuda.synchronize(device)
    assert (done.cpu().numpy().sum(1) == [0, 0, 0, 0, 0, N, 0, 0]).all()
    for a, b in zip(*before):
        assert (a == b).all()
    assert (before[0][0][inside] == bank[0][s]).all()  # its walls are the old level's to the end of its episode
    log, twin = (x.cpu().numpy() for x in logs)
    assert (twin[:6] == first[None, :]).all()
    assert (log[:cut] == twin[:cut]).all()
    assert (log[cut:6][:, inside] == -1).all() and (log[cut:6][:, ~inside] == twin[cut:6][:, ~inside]).all()
    second = LR.draws(LEVEL_SEED, 0, N, 1, 1, UNIFORM)[:, 0]
    assert (log[6:] == second[None, :]).all() and (twin[6:] == second[None, :]).all()  # the next map: drawn as before
    counts = [torch.zeros(N, dtype=torch.int32, device=device) for _ in range(2)]
    cur = [env.current_levels(counts=c).cpu().numpy() for env, c in zip(envs, counts)]
    assert (cur[0] == second).all() and (cur[1] == second).all()
    assert (counts[0] == 2).all() and (counts[1] == 2).all()
    # after the reset an env that drew s plays the child, every other env what its twin plays
    after = [tuple(x.cpu().numpy() for x in env.snapshot()) for env in envs]
    again = second == s
    assert again.any()
    for j in range(3):
        assert (after[0][j][~again] == after[1][j][~again]).all()
    assert (after[0][0][again] == kids[0][1]).all() and (after[0][1][again] == kids[1][1]).all()
    assert (after[1][0][again] == bank[0][s]).all()
    # the scores of the steps played on the old map credit nothing to s
    adv = torch.ones((4, N), dtype=torch.float32, device=device)
    _, c = nat.level_scores(adv, logs[0][cut:6].contiguous(), L, 0)
    c = c.cpu().numpy()
    assert c[s] == 0 and c.sum() == 4 * (N - inside.sum())
    _, c2 = nat.level_scores(adv, logs[1][cut:6].contiguous(), L, 0)
    assert c2.cpu().numpy()[s] == 4 * inside.sum()
    for env in envs:
        env.errors()
        env.close()


def test_captured_graph_plays_a_replaced_level(device):
    """max_steps 2, turns only: a four-step launch resets every env after its steps 1 and 3.  Captured under the old
    bank; a slot replaced afterwards reaches the replays through the bank's buffers."""
    from merlin import _native as nat

    bank, kids = maps()
    env = make_env(device, max_steps=2)
    env.reset()
    acts = torch.zeros((4, N), dtype=torch.int64, device=device)
    log = torch.full((4, N), -7, dtype=torch.int32, device=device)
    done = torch.zeros((4, N), dtype=torch.float32, device=device)
    env.set_level_log(log)
    env.step_into(acts, None, None, None, None, done, n_steps=4)  # eager (and the capture's warm-up)
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    with nat.capture_guard(), torch.cuda.graph(g):
        env.step_into(acts, None, None, None, None, done, n_steps=4)
    env.set_level_cdf(torch.from_numpy(LR.cdf_of(np.eye(L)[5])).to(device))
    g.replay()
    torch.cuda.synchronize(device)
    assert (log[2:] == 5).all() and (env.snapshot()[0].cpu().numpy() == bank[0][5]).all()
    env.replace_levels(i32(device, [5]), dev_kids(device, slice(2, 3)))
    g.replay()
    torch.cuda.synchronize(device)
    assert (done.cpu().numpy() == np.array([0, 1, 0, 1], dtype=np.float32)[:, None]).all()
    assert (log[:2] == -1).all() and (log[2:] == 5).all()  # the episode on the old map is no level's; then the child
    walls, goal, agent = (t.cpu().numpy() for t in env.snapshot())
    assert (walls == kids[0][2]).all() and (goal == kids[1][2]).all() and (agent == kids[2][2]).all()
    env.errors()
    env.close()


# ----------------------------------------------------------------------------------------------------------- trainer
PN, PT, PL, PC = 64, 16, 32, 8
_RUNS = {}


def _run(device, graph):
    from merlin import MerlinVecEnv
    from merlin.level_edit import LevelEditor
    from merlin.levels import LevelSampler, LevelSet
    from merlin.ppo import PPO

    ls = LevelSet.from_seeds(range(900, 900 + PL), difficulty="mediumhard", size=16, device=device)
    env = MerlinVecEnv(PN, "mediumhard", seed=777, device=device, max_steps=6)
    torch.manual_seed(0)
    sampler = LevelSampler(PL, "plr", beta=0.3, rho=0.2, device=device)
    editor = LevelEditor(PC, edits=4, seed=3)
    agent = PPO(env, batch_size=PN * PT, minibatch_size=PN * PT // 2, update_epochs=1, ent_coef=0.05, device=device,
                rollout_graph=graph, level_set=ls, level_sampler=sampler, level_seed=5, level_editor=editor)
    rows, graphs = [], []
    for it in (1, 2):
        lv = agent.collect_rollouts()
        graphs.append(agent._graph)
        agent.update(lv)
        torch.cuda.synchronize(device)
        st = agent.level_set
        rows.append(dict(
            bank=bank_np(env), set=tuple(t.cpu().numpy().copy() for t in (st.walls, st.goal, st.agent)),
            generation=st.generation.cpu().numpy().copy(), parent=st.parent.cpu().numpy().copy(),
            slots=editor.last_slots.cpu().numpy().copy(), parents=editor.last_parents.cpu().numpy().copy(),
            seen=sampler.seen.cpu().numpy().copy(), levels=agent.buf.levels.cpu().numpy().copy(),
            accepted=int(editor.accepted.item()), round=editor.generation, last=int(editor.last_accepted.item())))
    env.errors()
    return rows, graphs


def run(device, graph):
    if graph not in _RUNS:
        _RUNS[graph] = _run(device, graph)
    return _RUNS[graph]


def test_trainer_evolves_the_bank(device):
    rows, graphs = run(device, True)
    assert graphs[0] is not None and graphs[1] is graphs[0]  # captured once: the replacement needs no re-capture
    total = 0
    for it, row in enumerate(rows, 1):
        for a, b in zip(row["bank"], row["set"]):
            assert (a == b).all(), it
        assert row["round"] == it
        took = row["slots"] >= 0
        assert took.sum() == row["last"] and row["last"] > 0
        total += int(took.sum())
        assert row["accepted"] == total
        slots = row["slots"][took]
        assert len(set(slots.tolist())) == slots.size
        assert not row["seen"][slots].any()  # a replaced slot is an unseen level
        assert (row["generation"][slots] == it).all() and (row["parent"][slots] == row["parents"][took]).all()
        par = row["parents"][took]
        assert (par >= 0).all() and row["seen"][par].all() and not set(par.tolist()) & set(slots.tolist())
    assert (rows[0]["generation"] <= 1).all() and (rows[1]["generation"] <= 2).all()
    assert ((rows[1]["generation"] == 0) == (rows[1]["parent"] == -1)).all()
    # the second rollout (a replay of the graph) played children of the first round: unseen levels weigh 1 / L
    assert np.isin(rows[1]["levels"], rows[0]["slots"][rows[0]["slots"] >= 0]).any()


def test_trainer_graph_and_eager_build_the_same_bank(device):
    on, off = run(device, True)[0], run(device, False)[0]
    for k, (a, b) in enumerate(zip(on, off)):
        for f in ("generation", "parent", "slots", "parents", "seen", "levels"):
            assert (a[f] == b[f]).all(), (k, f)
        for x, y in zip(a["bank"], b["bank"]):
            assert (x == y).all(), k


def test_two_editors_on_the_same_scores_build_the_same_bank(device):
    """What data parallelism relies on: the edit key holds no rank, so ranks that hold the same (all-reduced) scores
    build the same bank bit for bit."""
    from merlin.level_edit import LevelEditor
    from merlin.levels import LevelSampler, LevelSet

    rs = np.random.RandomState(4)
    score, seen = rs.rand(PL), rs.rand(PL) < 0.8
    last = rs.randint(1, 4, PL)
    out = []
    for _ in range(2):
        ls = LevelSet.from_arrays(*R.bank([R.serpentine(16), R.open_room(16)] * (PL // 2)), device=device)
        sm = LevelSampler(PL, "plr", beta=0.3, rho=0.2, device=device)
        sm.score, sm.seen = torch.from_numpy(score).to(device), torch.from_numpy(seen).to(device)
        sm.last_seen, sm.iteration = torch.from_numpy(last).to(device), 3
        ed = LevelEditor(PC, edits=1, seed=9)
        slots = [ed.evolve(ls, sm, None, 3 + r).cpu().numpy() for r in range(2)]
        out.append((slots, [t.cpu().numpy() for t in (ls.walls, ls.goal, ls.agent, ls.generation, ls.parent)],
                    sm.seen.cpu().numpy(), [int(c.item()) for c in (ed.accepted, ed.rejected_unsolvable,
                                                                     ed.rejected_unchanged)]))
    a, b = out
    assert all((x == y).all() for x, y in zip(a[0], b[0])) and all((x == y).all() for x, y in zip(a[1], b[1]))
    assert (a[2] == b[2]).all() and a[3] == b[3]
    assert a[3][0] > 0 and sum(a[3]) == 2 * PC and (a[1][3] > 0).sum() > 0


def test_ppo_rejects_an_editor_without_plr(device):
    from merlin import MerlinVecEnv
    from merlin.level_edit import LevelEditor
    from merlin.levels import LevelSampler, LevelSet
    from merlin.ppo import PPO

    env = MerlinVecEnv(PN, "mediumhard", seed=777, device=device, max_steps=6)
    kw = dict(batch_size=PN * 2, minibatch_size=PN, device=device, level_editor=LevelEditor(2))
    with pytest.raises(ValueError):
        PPO(env, **kw)
    ls = LevelSet.from_seeds(range(900, 904), difficulty="mediumhard", size=16, device=device)
    with pytest.raises(ValueError):
        PPO(env, level_set=ls, level_sampler=LevelSampler(4, "uniform", device=device), **kw)
    env.close()
