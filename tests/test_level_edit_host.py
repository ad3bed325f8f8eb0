"""CPU: level editing's host side against tests/level_edit_ref.py -- the library's plain-C++ restatement of the edit rule
(merlin_levels_mutate_host) exactly, LevelSet.from_arrays on the children, the editor's selection logic and the
sampler's / set's masked updates against plain-Python restatements, the lineage's save / load round trip, and the new
entries' argument checks."""
import functools

import numpy as np
import pytest
import torch

import level_edit_ref as R
from pathing_ref import oracle_maps

EDITS = (0, 1, 4, 16, 64)
MAKERS = {"open": R.open_room, "serpentine": R.serpentine}


@functools.lru_cache(maxsize=None)
def reference(maker, S, E):
    """The reference's children of one hand-made map (64, the recorded key), computed once and never modified."""
    out = R.outcome(MAKERS[maker], S, E)
    for a in out:
        a.setflags(write=False)
    return out


def host(walls, goal, agent, parent_index, S, E, seed=R.EDIT_SEED, generation=R.GENERATION, count=None):
    from merlin import _native as nat

    return nat.levels_mutate_host(walls, goal, agent, parent_index, S, E, seed, generation, count=count)


def assert_same(got, ref):
    for name, g, r in zip(("walls", "goal", "agent", "dist", "changed"), got, ref):
        assert g.shape == r.shape and (g == r).all(), name


def test_reference_reaches_every_outcome():
    """On the reference alone: the inputs of the tests below hold every outcome class they rely on."""
    for S in (5, 7):
        _, _, _, dist, changed, noop = reference("serpentine", S, 1)
        assert (changed == 0).any() and (dist < 0).any() and (noop.sum(0) > 0).all(), S
        assert ((changed == 1) & (dist >= 0)).any(), S  # and accepted children
        _, _, _, dist, _, noop = reference("serpentine", S, 4)
        assert (dist < 0).any() and (noop.sum(0) > 0).all(), S
    # the counts recorded with the rule (edit_seed 7, generation 1, 64 children)
    _, _, _, dist, changed, noop = reference("serpentine", 5, 1)
    assert ((changed == 0).sum(), (dist < 0).sum(), *noop.sum(0)) == (17, 13, 6, 7, 4)
    _, _, _, dist, changed, noop = reference("serpentine", 7, 1)
    assert ((changed == 0).sum(), (dist < 0).sum(), *noop.sum(0)) == (16, 13, 2, 7, 7)
    for S in (16, 22, 32):
        _, _, _, dist, changed, _ = reference("serpentine", S, 1)
        assert (dist < 0).sum() >= 10 and (changed == 0).sum() >= 14, S
        _, _, _, dist, changed, _ = reference("open", S, 1)
        assert (dist < 0).sum() <= 1 and (changed == 0).sum() <= 1, S


@pytest.mark.parametrize("S", R.SIZES)
@pytest.mark.parametrize("E", EDITS)
@pytest.mark.parametrize("maker", sorted(MAKERS))
def test_host_equals_reference(maker, S, E):
    walls, goal, agent = R.bank([MAKERS[maker](S)])
    ref = reference(maker, S, E)
    got = host(walls, goal, agent, np.zeros(R.CHILDREN, dtype=np.int32), S, E)
    assert_same(got, ref[:5])
    if E == 0:
        assert (got[4] == 0).all() and (got[0] == walls[0]).all() and (got[3] == got[3][0]).all()
    # the border is never touched and the child is a valid level
    full, edge = (1 << S) - 1, 1 | (1 << (S - 1))
    assert (got[0][:, 0] == full).all() and (got[0][:, S - 1] == full).all() and ((got[0] & edge) == edge).all()


def test_toggles_cancel():
    """A child whose edits toggle one cell twice and change nothing else reports changed 0: constructed on the
    reference (5x5 room, 9 interior cells, 2 edits), then asked of the library."""
    S, E = 5, 2
    walls, goal, agent = R.bank([R.open_room(S)])
    pidx = np.zeros(2000, dtype=np.int32)
    ref = R.mutate(walls, goal, agent, pidx, pidx.size, S, E, 3, 2)
    cancel = (ref[4] == 0) & (ref[5].sum(1) == 0)  # unchanged without a no-op: two toggles of one cell
    assert cancel.any()
    got = host(walls, goal, agent, pidx, S, E, seed=3, generation=2)
    assert_same(got, ref[:5])


@pytest.mark.parametrize("diff,S", [("mediumhard", 16), ("hard", 22), ("easy", 5), ("hardest", 32)])
def test_host_equals_reference_on_generated_maps(oracle, diff, S):
    """Seed-built parents (the oracle's maps), each child from its own parent (parent_index NULL), E = 4."""
    _, walls, goal, agent = oracle_maps(oracle, diff, S, range(500, 512))
    ref = R.mutate(walls, goal, agent, None, 12, S, 4, 11, 3)
    assert_same(host(walls, goal, agent, None, S, 4, seed=11, generation=3), ref[:5])
    assert ref[4].any()


def test_parent_index_null_repeated_and_out_of_range():
    S, E = 7, 4
    walls, goal, agent = R.bank([R.serpentine(S), R.open_room(S), R.serpentine(S)])
    # NULL: child c from parent c, for C < P too
    for count in (3, 2):
        assert_same(host(walls, goal, agent, None, S, E, count=count),
                    R.mutate(walls, goal, agent, None, count, S, E, R.EDIT_SEED, R.GENERATION)[:5])
    pidx = np.array([2, 2, 0, -1, 3, 1, 1 << 30, -(1 << 31), 1, 0], dtype=np.int32)
    ref = R.mutate(walls, goal, agent, pidx, pidx.size, S, E, R.EDIT_SEED, R.GENERATION)
    got = host(walls, goal, agent, pidx, S, E)
    assert_same(got, ref[:5])
    bad = (pidx < 0) | (pidx >= 3)
    assert bad.sum() == 4
    assert (got[0][bad] == 0).all() and (got[1][bad] == 0).all() and (got[2][bad] == 0).all()
    assert (got[3][bad] == -1).all() and (got[4][bad] == 0).all()
    # the same parent under two child indices: two different keys
    assert not ((got[0][0] == got[0][1]).all() and (got[1][0] == got[1][1]).all() and (got[2][0] == got[2][1]).all())


def test_key():
    """The edits depend on (seed, generation, child index) only."""
    S = 16
    walls, goal, agent = R.bank([R.serpentine(S)])
    pidx = np.zeros(40, dtype=np.int32)
    a = host(walls, goal, agent, pidx, S, 4)
    b = host(walls, goal, agent, pidx[:17], S, 4)
    assert all((x[:17] == y).all() for x, y in zip(a, b))
    for kw in (dict(seed=8), dict(generation=2)):
        c = host(walls, goal, agent, pidx, S, 4, **kw)
        assert any((x != y).any() for x, y in zip(a[:3], c[:3]))
    big = host(walls, goal, agent, pidx, S, 4, seed=(1 << 64) - 1, generation=(1 << 63) + 5)
    assert_same(big, R.mutate(walls, goal, agent, pidx, 40, S, 4, (1 << 64) - 1, (1 << 63) + 5)[:5])


def test_invalid_arguments():
    from merlin import _native as nat

    L = nat.lib()
    S = 7
    walls, goal, agent = R.bank([R.serpentine(S)])
    pidx = np.zeros(4, dtype=np.int32)
    out = (np.zeros((4, S), np.uint32), np.zeros((4, 2), np.int32), np.zeros((4, 4), np.int32),
           np.full(4, 77, np.int32), np.full(4, 77, np.uint8))
    p = nat.np_ptr

    def call(size=S, edits=1, P=1, Cn=4, w=walls, g=goal, a=agent, pi=pidx, outs=out):
        return L.merlin_levels_mutate_host(p(w), p(g), p(a), P, p(pi), Cn, size, edits, 1, 1, *(p(o) for o in outs))

    assert call() == nat.MERLIN_OK
    for kw in (dict(size=4), dict(size=33), dict(edits=-1), dict(edits=65), dict(Cn=-1), dict(P=-1), dict(w=None),
               dict(g=None), dict(a=None), dict(pi=None, Cn=2),  # NULL index: C <= P
               *(dict(outs=tuple(None if j == k else o for j, o in enumerate(out))) for k in range(5))):
        assert call(**kw) == nat.E_INVALID, kw
    assert call(pi=None, Cn=1) == nat.MERLIN_OK
    # C = 0: nothing to do, whatever the pointers
    out[3][:] = 77
    assert call(Cn=0, w=None, outs=(None,) * 5) == nat.MERLIN_OK and (out[3] == 77).all()
    for s in ("merlin_levels_mutate", "merlin_levels_mutate_host", "merlin_env_replace_levels",
              "merlin_env_level_bank"):
        assert s in nat.EXPORTED_SYMBOLS and getattr(L, s).argtypes is not None
    # the device entry validates before it launches: the same codes without a GPU
    assert L.merlin_levels_mutate(None, None, None, 1, None, 4, 4, 1, 1, 1, None, None, None, None, None,
                                  None) == nat.E_INVALID
    assert L.merlin_levels_mutate(None, None, None, 1, None, 4, S, 1, 1, 1, None, None, None, None, None,
                                  None) == nat.E_INVALID
    assert L.merlin_levels_mutate(None, None, None, 1, None, 0, S, 1, 1, 1, None, None, None, None, None,
                                  None) == nat.MERLIN_OK
    assert L.merlin_env_replace_levels(None, None, None, None, None, 1, None) == nat.E_INVALID
    assert L.merlin_env_level_bank(None, None, None, None, None) == nat.E_INVALID


@pytest.mark.parametrize("S", [5, 7, 16])
def test_from_arrays_accepts_exactly_the_solvable_children(S):
    from merlin.levels import LevelSet

    ow, og, oa, dist, _, _ = reference("serpentine", S, 1)
    assert (dist < 0).any() and (dist >= 0).any()
    LevelSet.from_arrays(ow, og, oa)  # every child is a valid level
    for c in range(R.CHILDREN):
        one = (ow[c:c + 1], og[c:c + 1], oa[c:c + 1])
        if dist[c] >= 0:
            LevelSet.from_arrays(*one, solvable=True)
        else:
            with pytest.raises(ValueError, match="cannot be reached"):
                LevelSet.from_arrays(*one, solvable=True)


# ---- selection ------------------------------------------------------------------------------------------------------
def make_sampler(score, seen, last_seen, iteration, beta=0.3, rho=0.2):
    from merlin.levels import LevelSampler

    sm = LevelSampler(len(score), "plr", beta=beta, rho=rho, device="cpu")
    sm.score = torch.tensor(score, dtype=torch.float64)
    sm.seen = torch.tensor(seen, dtype=torch.bool)
    sm.last_seen = torch.tensor(last_seen, dtype=torch.int64)
    sm.iteration = iteration
    return sm


SELECT_CASES = {
    # score, seen, last_seen
    "plain": ([.5, .1, .9, .3, .7, .2, .8, .4], [1] * 8, [3, 1, 3, 2, 3, 1, 2, 3]),
    "ties": ([.5, .5, .5, .1, .1, .9, .9, .1], [1] * 8, [3] * 8),
    "unseen": ([.5, .0, .9, .0, .7, .2, .0, .4], [1, 0, 1, 0, 1, 1, 0, 1], [3, 0, 3, 0, 2, 1, 0, 3]),
    "few_seen": ([.0, .0, .9, .0, .7, .0, .0, .0], [0, 0, 1, 0, 1, 0, 0, 0], [0, 0, 3, 0, 3, 0, 0, 0]),
    "one_seen": ([.0, .0, .0, .0, .7, .0, .0, .0], [0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 3, 0, 0, 0]),
    "none_seen": ([.0] * 8, [0] * 8, [0] * 8),
}


@pytest.mark.parametrize("name", sorted(SELECT_CASES))
@pytest.mark.parametrize("children", [1, 3, 5, 8])
def test_selection_equals_restatement(name, children):
    from merlin.level_edit import select_parents, select_victims

    score, seen, last = SELECT_CASES[name]
    sm = make_sampler(score, seen, last, 3)
    parents, ok = select_parents(sm, children)
    ref_p = R.parents_ref(score, seen, children)
    assert [(int(l), bool(o)) for l, o in zip(parents, ok)] == ref_p
    victims = select_victims(sm, parents, ok, children)
    ref_v = R.victims_ref(sm.weights().tolist(), seen, ref_p, children)
    assert victims.tolist() == ref_v
    # a parent is never its own round's victim; victims are distinct seen levels
    real = [v for v in ref_v if v >= 0]
    assert not set(real) & {l for l, o in ref_p if o} and len(set(real)) == len(real) and all(seen[v] for v in real)
    n_el = sum(seen) - sum(o for _, o in ref_p)
    assert len(real) == min(children, n_el)  # fewer eligible levels than children: the rest are -1


def test_selection_cases_cover_what_they_claim():
    score, seen, _ = SELECT_CASES["ties"]
    assert R.parents_ref(score, seen, 3) == [(5, True), (6, True), (0, True)]  # ties to the lower index
    sm = make_sampler(*SELECT_CASES["ties"], 3)
    w = sm.weights().tolist()
    assert R.victims_ref(w, seen, R.parents_ref(score, seen, 3), 3) == [7, 4, 3]  # the lowest ranks, lowest first
    score, seen, _ = SELECT_CASES["few_seen"]
    assert R.victims_ref([1 / 8] * 8, seen, R.parents_ref(score, seen, 1), 3) == [4, -1, -1]
    assert [o for _, o in R.parents_ref(score, seen, 3)] == [True, True, False]


def test_forget_ignores_minus_one():
    sm = make_sampler(*SELECT_CASES["plain"], 3)
    before = (sm.score.clone(), sm.seen.clone(), sm.last_seen.clone())
    sm.forget(torch.tensor([-1, -1], dtype=torch.int32))
    assert all((a == b).all() for a, b in zip(before, (sm.score, sm.seen, sm.last_seen)))
    sm.forget(torch.tensor([6, -1, 0], dtype=torch.int32))
    hit = torch.zeros(8, dtype=torch.bool)
    hit[[0, 6]] = True
    assert (sm.seen == ~hit).all() and (sm.score[hit] == 0).all() and (sm.last_seen[hit] == 0).all()
    assert (sm.score[~hit] == before[0][~hit]).all() and (sm.last_seen[~hit] == before[2][~hit]).all()
    w = sm.weights()
    assert (w[hit] == 1.0 / 8).all() and abs(float(w.sum()) - 1.0) < 1e-12  # unseen: 1 / L each
    assert float(sm.cdf()[-1]) == 1.0


def test_replace_ignores_minus_one_and_is_in_place():
    from merlin.levels import LevelSet

    S = 7
    parents = LevelSet.from_arrays(*R.bank([R.serpentine(S), R.open_room(S)] * 3))
    ow, og, oa, _, _, _ = reference("serpentine", S, 4)
    kids = LevelSet.from_arrays(ow[:4], og[:4], oa[:4])
    held = (parents.walls, parents.goal, parents.agent, parents.generation, parents.parent)
    before = [t.clone() for t in held]
    assert (parents.generation == 0).all() and (parents.parent == -1).all()
    parents.replace_(torch.tensor([-1, -1, -1, -1], dtype=torch.int32), kids, 5, torch.zeros(4, dtype=torch.int32))
    assert all((a == b).all() for a, b in zip(before, held))
    slots = torch.tensor([4, -1, 0, -1], dtype=torch.int32)
    parents.replace_(slots, kids, 5, torch.tensor([2, 9, 3, 9], dtype=torch.int32))
    assert all(a is b for a, b in zip(held, (parents.walls, parents.goal, parents.agent, parents.generation,
                                              parents.parent)))  # the same tensors: every holder sees the change
    for j, s in ((0, 4), (2, 0)):
        assert (parents.walls[s] == kids.walls[j]).all() and (parents.goal[s] == kids.goal[j]).all()
        assert (parents.agent[s] == kids.agent[j]).all()
    assert parents.generation.tolist() == [5, 0, 0, 0, 5, 0] and parents.parent.tolist() == [3, -1, -1, -1, 2, -1]
    for s in (1, 2, 3, 5):
        assert all((t[s] == b[s]).all() for t, b in zip(held, before))


def test_lineage_save_load(tmp_path):
    from merlin.levels import LevelSet

    S = 7
    ls = LevelSet.from_arrays(*R.bank([R.serpentine(S), R.open_room(S), R.serpentine(S)]))
    ls.generation.copy_(torch.tensor([0, 4, 2], dtype=torch.int32))
    ls.parent.copy_(torch.tensor([-1, 2, 0], dtype=torch.int32))
    path = str(tmp_path / "bank.npz")
    ls.save(path)
    back = LevelSet.load(path)
    assert back.generation.tolist() == [0, 4, 2] and back.parent.tolist() == [-1, 2, 0]
    assert back.generation.dtype == back.parent.dtype == torch.int32
    assert (back.walls == ls.walls).all() and (back.goal == ls.goal).all() and (back.agent == ls.agent).all()
    # a file written before level editing: no lineage arrays, the defaults
    old = str(tmp_path / "old.npz")
    np.savez(old, walls=ls.walls.numpy(), goal=ls.goal.numpy(), agent=ls.agent.numpy(), size=np.int32(S))
    back = LevelSet.load(old)
    assert back.generation.tolist() == [0, 0, 0] and back.parent.tolist() == [-1, -1, -1]
    moved = back.to("cpu")
    assert moved.generation.tolist() == [0, 0, 0]


def test_editor_arguments():
    from merlin.level_edit import LevelEditor

    for kw in (dict(children=0), dict(children=2, edits=65), dict(children=2, edits=-1), dict(children=2, every=0)):
        with pytest.raises(ValueError):
            LevelEditor(**kw)
    ed = LevelEditor(4, edits=2, every=3)
    assert [ed.due(i) for i in (1, 2, 3, 6)] == [False, False, True, True]
