"""GPU parity of mixed-task vector envs (per-env generator classes, merlin_env_set_difficulties) against the C oracle.

The oracle steps envs independently, so a mixed batch is checked class by class: for class d, the envs idx of that
class against oracle.batch_rollout(seeds[idx], actions[:, idx], difficulty=d) / oracle.gen_map(size, d, seed).

n = 300 envs: the last step block (128 envs) and the last reset block (64) are partial.  Sizes 9 (the smallest at
which all five generators run, SP = 16 with padded rows), 16 (SP = 16 full) and 17 (SP = 32).  Two assignments:
interleaved i % 5 (every wave holds all five classes) and runs of 70/50/64/66/50 (boundaries inside waves).
The reference rollouts are computed once per (size, assignment) and shared by the modes."""
import numpy as np
import pytest
import torch

from minigrid_literal import LiteralEnv

pytestmark = pytest.mark.gpu

N = 300
T, MAX_STEPS = 120, 40
P_FWD = [0.15, 0.15, 0.7]
NAMES = ["easy", "medium", "mediumhard", "hard", "hardest"]
SIZES = [9, 16, 17]


def assignment(kind):
    if kind == "interleaved":
        return [NAMES[i % 5] for i in range(N)]
    runs = [70, 50, 64, 66, 50]
    assert sum(runs) == N
    return [d for d, r in zip(NAMES, runs) for _ in range(r)]


CASES = [(s, k) for s in SIZES for k in ("interleaved", "runs")]
IDS = [f"{s}-{k}" for s, k in CASES]


def unpack(codes_i32: torch.Tensor) -> np.ndarray:
    """int32[..., 8] nibble words -> uint8[..., 49] tile classes."""
    w = codes_i32.cpu().numpy().astype(np.uint32).view(np.uint32)
    nib = (w[..., :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xF
    return nib.reshape(*w.shape[:-1], 64)[..., :49].astype(np.uint8)


def make_env(names, size, seed, device, n=N, **kw):
    from merlin import MerlinVecEnv

    return MerlinVecEnv(n, difficulty=names, size=size, seed=seed, device=device, **kw)


def base_of(size):
    return 555 + 1000 * size


def seeds_of(base, n=N):
    return np.arange(base, base + n, dtype=np.uint64)


def actions(seed, steps=T, n=N):
    return np.random.RandomState(seed).choice([0, 1, 2], size=(steps, n), p=P_FWD).astype(np.int64)


def class_indices(names):
    names = np.asarray(names)
    return {d: np.flatnonzero(names == d) for d in NAMES if (names == d).any()}


def assert_maps(oracle, st, names, size, seeds, envs=None):
    """The state of each env against oracle.gen_map of its own class and seed."""
    for i in (range(len(names)) if envs is None else envs):
        cells, meta = oracle.gen_map(size, names[i], int(seeds[i]))
        assert (st["cells"][i] == cells).all(), (size, i, names[i])
        assert tuple(st["agent_pos"][i]) == tuple(meta[0:2]) and st["agent_dir"][i] == meta[2], (size, i)
        assert tuple(st["goal_pos"][i]) == tuple(meta[3:5]), (size, i)


_REF = {}


def reference(oracle, size, kind):
    """(names, actions, codes [T+1], reward, term, trunc) of the mixed batch, assembled class by class; computed once
    per (size, assignment) and never modified."""
    key = (size, kind)
    if key not in _REF:
        names = assignment(kind)
        acts = actions(size)
        seeds = seeds_of(base_of(size))
        codes = np.zeros((T + 1, N, 49), dtype=np.uint8)
        rew = np.zeros((T, N), dtype=np.float32)
        term = np.zeros((T, N), dtype=np.uint8)
        trunc = np.zeros((T, N), dtype=np.uint8)
        for d, idx in class_indices(names).items():
            oc, orew, ote, otr, _ = oracle.batch_rollout(seeds[idx], np.ascontiguousarray(acts[:, idx]), size=size,
                                                         difficulty=d, max_steps=MAX_STEPS)
            codes[:, idx], rew[:, idx], term[:, idx], trunc[:, idx] = oc, orew, ote, otr
        # every env auto-resets at least twice, and both kinds of episode end occur
        assert (np.maximum(term, trunc).sum(0) >= 2).all() and trunc.sum() > 0 and term.sum() > 0
        for a in (codes, rew, term, trunc, acts):
            a.setflags(write=False)
        _REF[key] = (names, acts, codes, rew, term, trunc)
    return _REF[key]


def no_errors(env):
    flags, _ = env.errors()
    assert flags == 0


@pytest.mark.parametrize("size,kind", CASES, ids=IDS)
def test_seeded_reset_maps(oracle, device, size, kind):
    names = assignment(kind)
    env = make_env(names, size, base_of(size), device)
    assert env.difficulty == "mixed" and env.difficulties == names
    ids = env.class_ids.cpu().numpy()
    assert ids.dtype == np.uint8 and (ids == [NAMES.index(d) for d in names]).all()
    env.reset()
    assert_maps(oracle, env.get_state(), names, size, seeds_of(base_of(size)))
    no_errors(env)
    env.close()


@pytest.mark.parametrize("mode", ["default_refill", "refill_every_step", "fallback_only", "multi_step"])
@pytest.mark.parametrize("size,kind", CASES, ids=IDS)
def test_rollout_vs_oracle(oracle, device, size, kind, mode):
    """Codes, reward, term and trunc of 120 auto-resetting steps, bit-exact, through each path that generates a map:
    the periodic refill (k_env_refill<SP, 4>), a refill after every step, no refill at all (k_env_fallback), and one
    multi-step launch (the generator inside k_env_step<SP, false>)."""
    names, acts, ocodes, orew, oterm, otrunc = reference(oracle, size, kind)
    env = make_env(names, size, base_of(size), device, max_steps=MAX_STEPS)
    if mode in ("refill_every_step", "fallback_only"):
        env.set_refill_interval(0)
    obs0 = unpack(env.reset().clone())
    codes = torch.zeros((T, N, 8), dtype=torch.int32, device=device)
    rew = torch.zeros((T, N), dtype=torch.float32, device=device)
    term = torch.zeros((T, N), dtype=torch.uint8, device=device)
    trunc = torch.zeros((T, N), dtype=torch.uint8, device=device)
    ta = torch.from_numpy(acts.copy()).to(device)
    if mode == "multi_step":
        env.step_into(ta, codes, rew, term, trunc, None, n_steps=T, action_stride=N)
    else:
        for t in range(T):
            env.step_into(ta[t], codes[t], rew[t], term[t], trunc[t], None)
            if mode == "refill_every_step":
                env.refill()
    assert (obs0 == ocodes[0]).all()
    assert (unpack(codes) == ocodes[1:]).all()
    assert (rew.cpu().numpy() == orew).all()
    assert (term.cpu().numpy() == oterm).all() and (trunc.cpu().numpy() == otrunc).all()
    no_errors(env)
    env.close()


@pytest.mark.parametrize("size", [9, 17])
def test_reseed_each_reset_mixed(oracle, device, size):
    """reseed_each_reset with mixed classes: every episode of env i restarts on gen_map(size, diff_i, seed_i) -- the
    observation after every episode end is the first one again, the walls stay the seed's map of the env's class,
    and an explicit reset gives its agent again."""
    steps, max_steps = 63, 7
    names = assignment("interleaved")
    seeds = seeds_of(900 + size)
    env = make_env(names, size, None, device, seeds=seeds, reseed_each_reset=True, max_steps=max_steps)
    obs0 = unpack(env.reset().clone())
    assert_maps(oracle, env.get_state(), names, size, seeds)
    codes = torch.zeros((steps, N, 8), dtype=torch.int32, device=device)
    done = torch.zeros((steps, N), dtype=torch.float32, device=device)
    ta = torch.from_numpy(actions(size, steps)).to(device)
    for t in range(steps):
        env.step_into(ta[t], codes[t], None, None, None, done[t])
    ends = done.cpu().numpy() > 0
    assert ends.sum() > 3 * N
    codes = unpack(codes)
    assert (codes[ends] == np.broadcast_to(obs0, codes.shape)[ends]).all()
    st = env.get_state()
    for i, s in enumerate(seeds):
        cells, meta = oracle.gen_map(size, names[i], int(s))
        assert ((st["cells"][i] == 1) == (cells == 1)).all() and tuple(st["goal_pos"][i]) == tuple(meta[3:5]), i
    assert (unpack(env.reset()) == obs0).all()
    assert_maps(oracle, env.get_state(), names, size, seeds)
    no_errors(env)
    env.close()


@pytest.mark.parametrize("size", [9, 17])
def test_reassignment_takes_effect_at_next_map(oracle, device, size):
    """set_difficulties leaves the envs' current maps alone; each env's next auto-reset map is the NEW class's map
    drawn from the env's continued RNG stream.  The literal model gives that map: reset(seed) with the old class,
    then an unseeded reset with the new one (the steps in between draw nothing).  Every 4th env against the literal
    model (it is Python); then, after a reseed, every env's next map against oracle.gen_map of the new class."""
    max_steps = 5
    old = assignment("interleaved")
    new = [NAMES[(i + 2) % 5] for i in range(N)]
    base = 70 + size
    env = make_env(old, size, base, device, max_steps=max_steps)
    env.reset()
    st0 = env.get_state()
    env.set_difficulties(new)
    assert env.difficulties == new
    st1 = env.get_state()
    for k in ("walls", "agent_pos", "agent_dir", "goal_pos", "rng"):
        assert (st1[k] == st0[k]).all(), k
    turn = torch.zeros(N, dtype=torch.int64, device=device)  # turning never reaches the goal: truncation at step 5
    trunc = torch.zeros(N, dtype=torch.uint8, device=device)
    for _ in range(max_steps):
        env.step_into(turn, None, None, None, trunc, None)
    assert bool(trunc.all())
    st2 = env.get_state()
    for i in range(0, N, 4):
        lit = LiteralEnv(size, old[i])
        lit.reset(seed=base + i)
        lit.difficulty = new[i]
        lit.reset()
        assert (st2["cells"][i] == lit.cells()).all(), (i, old[i], new[i])
        assert tuple(st2["agent_pos"][i]) == tuple(lit.agent_pos) and st2["agent_dir"][i] == lit.agent_dir, i
    # a reseed right after a switch: the next auto-reset map is gen_map of the new class and the new seed
    newer = [NAMES[(i + 3) % 5] for i in range(N)]
    seeds = seeds_of(31000 + size)
    env.set_difficulties(newer)
    env.seed_each(seeds)
    for _ in range(max_steps):
        env.step_into(turn, None, None, None, trunc, None)
    assert bool(trunc.all())
    assert_maps(oracle, env.get_state(), newer, size, seeds)
    no_errors(env)
    env.close()


def test_uniform_list_equals_string(device):
    """difficulty=["hard"] * n gives bitwise the same rollout as difficulty="hard"."""
    size, steps = 16, 96
    acts = torch.from_numpy(actions(3, steps)).to(device)
    outs = []
    for diff in ("hard", ["hard"] * N):
        env = make_env(diff, size, 4321, device, max_steps=12)
        assert env.difficulty == "hard" and env.difficulties == ["hard"] * N
        assert env.per_env_classes == (not isinstance(diff, str))
        obs0 = env.reset().clone()
        codes = torch.zeros((steps, N, 8), dtype=torch.int32, device=device)
        rew = torch.zeros((steps, N), dtype=torch.float32, device=device)
        term = torch.zeros((steps, N), dtype=torch.uint8, device=device)
        trunc = torch.zeros((steps, N), dtype=torch.uint8, device=device)
        epr = torch.zeros((steps, N), dtype=torch.float64, device=device)
        for t in range(steps):
            env.step_into(acts[t], codes[t], rew[t], term[t], trunc[t], None, epr[t])
        outs.append((obs0, codes, rew, term, trunc, epr, torch.from_numpy(env.get_state()["rng"].astype(np.int64))))
        no_errors(env)
        env.close()
    assert outs[0][3].sum() > 0 and outs[0][4].sum() > N
    for a, b in zip(*outs):
        assert torch.equal(a.cpu(), b.cpu())


def test_string_difficulty_never_calls_the_entry_point(device, monkeypatch):
    from merlin import _native as nat

    calls = []
    real = nat.lib().merlin_env_set_difficulties

    class Spy:
        def __getattr__(self, name):
            if name == "merlin_env_set_difficulties":
                calls.append(name)
                return real
            return getattr(nat._lib, name)

    spy = Spy()
    monkeypatch.setattr(nat, "lib", lambda: spy)
    env = make_env("medium", 16, 1, device, n=8)
    env.reset()
    assert calls == [] and env.per_env_classes is False
    env.set_difficulties(["easy"] * 8)
    assert calls == ["merlin_env_set_difficulties"]
    env.close()


def test_validation(device):
    from merlin import MerlinVecEnv
    from merlin import _native as nat

    with pytest.raises(ValueError):
        MerlinVecEnv(4, difficulty=["easy", "medium", "nope", "hard"], size=16, device=device)
    with pytest.raises(ValueError):
        MerlinVecEnv(4, difficulty=["easy", "medium", "hard"], size=16, device=device)
    with pytest.raises(nat.MerlinNativeError) as ei:
        MerlinVecEnv(4, difficulty=["easy", "medium", "hardest", "hard"], size=6, device=device)
    assert ei.value.code == nat.E_UNSUPPORTED == 4
    env = MerlinVecEnv(4, difficulty="easy", size=16, seed=5, device=device)
    with pytest.raises(ValueError):
        env.set_difficulties(["easy"] * 5)
    with pytest.raises(nat.MerlinNativeError) as ei:
        env.set_class_ids([0, 1, 7, 2])  # a raw id outside MERLIN_EASY..MERLIN_HARDEST
    assert ei.value.code == nat.E_INVALID == 1
    with pytest.raises(nat.MerlinNativeError) as ei:
        env.set_class_ids([0, 1, 2])  # n != num_envs
    assert ei.value.code == nat.E_INVALID
    # the failed calls changed nothing
    assert env.difficulty == "easy" and env.per_env_classes is False
    env.reset()
    no_errors(env)
    env.close()
