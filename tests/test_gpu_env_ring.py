"""GPU: the ring of look-ahead maps per env (merlin_env_set_lookahead_depth) changes no result, and PPO's rollout on it
equals the one-slot rollout bit for bit.

Env cases: n = 200 envs (three full waves and a partial one, a partial 128-env step block), T = 48 steps,
max_steps = 6, forward-biased actions: truncation alone ends at least 8 episodes per env, so every ring of depth <= 7
drains and wraps whatever the actions do.  Codes, rewards and dones are compared with oracle.batch_rollout, whose
result is computed once per (size, difficulty) and never modified.
PPO cases: 128 envs x 16 steps, max_steps 12 (the shape of tests/test_gpu_capture_safety.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T, MAX_STEPS = 200, 48, 6
BASE = 4242
DIFF_OF = {5: "mediumhard", 16: "mediumhard", 22: "hard"}  # SP = 16 (padded rows), SP = 16 full, SP = 32


def unpack(codes_i32: torch.Tensor) -> np.ndarray:
    """int32[..., 8] nibble words -> uint8[..., 49] tile classes."""
    w = codes_i32.cpu().numpy().astype(np.uint32).view(np.uint32)
    nib = (w[..., :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xF
    return nib.reshape(*w.shape[:-1], 64)[..., :49].astype(np.uint8)


def seeds_of(base):
    return np.arange(base, base + N, dtype=np.uint64)


def actions():
    return np.random.RandomState(5).choice([0, 1, 2], size=(T, N), p=[0.1, 0.1, 0.8]).astype(np.int64)


_REF = {}


def reference(oracle, size, difficulty=None, base=BASE):
    """(actions, codes [T+1], reward, done) of the oracle's rollout; `difficulty`: one name or N names."""
    names = [difficulty or DIFF_OF[size]] * N if not isinstance(difficulty, list) else difficulty
    key = (size, tuple(names), base)
    if key not in _REF:
        acts, seeds = actions(), seeds_of(base)
        codes = np.zeros((T + 1, N, 49), dtype=np.uint8)
        rew = np.zeros((T, N), dtype=np.float32)
        done = np.zeros((T, N), dtype=np.float32)
        for d in sorted(set(names)):
            idx = np.flatnonzero(np.asarray(names) == d)
            oc, orew, ote, otr, _ = oracle.batch_rollout(seeds[idx], np.ascontiguousarray(acts[:, idx]), size=size,
                                                         difficulty=d, max_steps=MAX_STEPS)
            codes[:, idx], rew[:, idx], done[:, idx] = oc, orew, np.maximum(ote, otr)
        assert (done.sum(0) >= 8).all()  # every ring of depth <= 7 drains
        for a in (acts, codes, rew, done):
            a.setflags(write=False)
        _REF[key] = (acts, codes, rew, done)
    return _REF[key]


def make_env(device, size, difficulty=None, seed=BASE, **kw):
    from merlin import MerlinVecEnv

    return MerlinVecEnv(N, difficulty=difficulty or DIFF_OF[size], size=size, seed=seed, device=device,
                        max_steps=MAX_STEPS, **kw)


def rollout(env, acts, device, steps=T, after_step=None, multi=False):
    """reset, then `steps` auto-resetting steps (one launch each, or one multi-step launch): obs0, codes, rew, done."""
    obs0 = unpack(env.reset().clone())
    codes = torch.zeros((steps, N, 8), dtype=torch.int32, device=device)
    rew = torch.zeros((steps, N), dtype=torch.float32, device=device)
    done = torch.zeros((steps, N), dtype=torch.float32, device=device)
    ta = torch.from_numpy(acts[:steps].copy()).to(device)
    if multi:
        env.step_into(ta, codes, rew, None, None, done, n_steps=steps, action_stride=N)
    else:
        for t in range(steps):
            env.step_into(ta[t], codes[t], rew[t], None, None, done[t])
            if after_step is not None:
                after_step(t)
    return obs0, unpack(codes), rew.cpu().numpy(), done.cpu().numpy()


def assert_equal(got, ref, steps=T):
    obs0, codes, rew, done = got
    _, ocodes, orew, odone = ref
    assert (obs0 == ocodes[0]).all()
    assert (codes == ocodes[1:steps + 1]).all()
    assert (rew == orew[:steps]).all()
    assert (done == odone[:steps]).all()


def no_errors(env):
    flags, _ = env.errors()
    assert flags == 0


def full_ring(env, depth):
    """Depth `depth`, refills the caller's, every ring full (seeding drops the maps, so the seeds go first)."""
    env.set_refill_interval(0)
    env.set_lookahead_depth(depth)
    env.ensure_seeded()
    env.refill()


@pytest.mark.parametrize("depth,size", [(2, 16), (3, 16), (7, 16), (2, 22), (3, 22), (7, 22), (3, 5)])
def test_ring_drains_then_fallback(oracle, device, depth, size):
    """A full ring, no top-up: the first `depth` resets of an env take the ring's maps in order, every later one
    generates in k_env_fallback from the state the last map left."""
    ref = reference(oracle, size)
    env = make_env(device, size)
    full_ring(env, depth)
    assert_equal(rollout(env, ref[0], device), ref)
    no_errors(env)
    env.close()


@pytest.mark.parametrize("mode", ["every_step", "every_5_steps"])
def test_ring_wraps_under_top_ups(oracle, device, mode):
    """Depth 3 topped up in-stream: by the caller after every step (one wave per 64 envs), or by the library every
    5 step launches (the packed SPAN 4 pass; rings drain and fall back in between).  8+ resets per env wrap the
    consume index several times."""
    ref = reference(oracle, 16)
    env = make_env(device, 16)
    full_ring(env, 3)
    if mode == "every_5_steps":
        env.set_refill_interval(5)
    got = rollout(env, ref[0], device, after_step=(lambda t: env.refill()) if mode == "every_step" else None)
    assert_equal(got, ref)
    no_errors(env)
    env.close()


@pytest.mark.parametrize("size", [16, 22])
def test_ring_of_rollout_depth_needs_no_fallback(oracle, device, size):
    """PPO's mode: depth T + 1 filled once, then the reset and T steps with the fallback pass off: no reset meets an
    empty ring (errors() would report MERLIN_DEVERR_SLOT_EMPTY)."""
    ref = reference(oracle, size)
    env = make_env(device, size)
    full_ring(env, T + 1)
    env.set_step_fallback(False)
    assert_equal(rollout(env, ref[0], device), ref)
    no_errors(env)
    env.close()


def test_ring_multi_step_launch(oracle, device):
    """Depth 4 under one n_steps = T launch: resets take the ring inside the step kernel, then generate in place."""
    ref = reference(oracle, 16)
    env = make_env(device, 16)
    full_ring(env, 4)
    assert_equal(rollout(env, ref[0], device, multi=True), ref)
    no_errors(env)
    env.close()


def test_seed_empties_the_ring(oracle, device):
    """A full ring of depth 4 holds maps of the old seeds: merlin_env_seed drops them all."""
    ref = reference(oracle, 16, base=BASE + 1000)
    env = make_env(device, 16)
    full_ring(env, 4)
    env.seed_each(seeds_of(BASE + 1000))
    assert_equal(rollout(env, ref[0], device, steps=20), ref, steps=20)
    no_errors(env)
    env.close()


def test_set_difficulties_empties_the_ring(oracle, device):
    """A full ring of depth 4 holds maps of the old class: merlin_env_set_difficulties drops them all (the envs'
    RNG streams stay: still the seeds' states here, as nothing was reset yet)."""
    names = [("mediumhard", "hard")[(i // 50) % 2] for i in range(N)]  # runs of 50: boundaries inside waves
    ref = reference(oracle, 16, difficulty=names)
    env = make_env(device, 16)
    full_ring(env, 4)
    env.set_difficulties(names)
    env.refill()  # the ring again, of the new classes
    assert_equal(rollout(env, ref[0], device, steps=20), ref, steps=20)
    no_errors(env)
    env.close()


def test_reseed_mode_reads_the_head_only(device):
    """reseed_each_reset: every reset is the seed's map again, the ring's head read and never advanced -- depth 4
    equals depth 1 bit for bit."""
    acts = actions()
    runs = []
    for depth in (1, 4):
        env = make_env(device, 16, seed=None, seeds=seeds_of(BASE), reseed_each_reset=True)
        env.set_lookahead_depth(depth)
        runs.append(rollout(env, acts, device))
        no_errors(env)
        env.close()
    for a, b in zip(*runs):
        assert (a == b).all()
    obs0, codes, _, done = runs[1]
    ends = done > 0
    assert ends.sum() >= 8 * N and (codes[ends] == np.broadcast_to(obs0, codes.shape)[ends]).all()


# ---------------------------------------------------------------------------------------------------------- PPO
PN, PT = 128, 16
FIELDS = ("codes", "actions", "logprobs", "values", "rewards", "dones", "ep_return", "ep_length", "last_value")


def _agent(device, ring):
    from merlin import MerlinVecEnv
    from merlin.ppo import PPO

    env = MerlinVecEnv(PN, "mediumhard", seed=777, device=device, max_steps=12)
    torch.manual_seed(0)
    agent = PPO(env, batch_size=PN * PT, minibatch_size=PN * PT // 4, update_epochs=1, ent_coef=0.05, device=device)
    assert agent.set_map_ring(ring) == ring
    assert agent.vec.lookahead_depth == (PT + 1 if ring else 1)
    return agent


def _three_rollouts(device, ring):
    """eager (+ capture), the first replay, a second replay, an update after each: every buffer field of every
    rollout and the parameters at the end."""
    agent = _agent(device, ring)
    bufs = []
    for _ in range(3):
        lv = agent.collect_rollouts()
        torch.cuda.synchronize(device)
        bufs.append({f: getattr(agent.buf, f).clone() for f in FIELDS})
        agent.update(lv)
    assert agent._graph is not None
    agent.vec.errors()
    return bufs, [p.detach().clone() for p in agent.ac.parameters()]


def test_ppo_rollouts_equal_with_and_without_the_ring(device):
    on, p_on = _three_rollouts(device, True)
    off, p_off = _three_rollouts(device, False)
    for k, (a, b) in enumerate(zip(on, off)):
        for f in FIELDS:
            assert torch.equal(a[f], b[f]), (k, f)
    assert (on[2]["dones"].sum(0) >= 1).all()  # every env reset inside a rollout
    for a, b in zip(p_on, p_off):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ring", [True, False], ids=["ring", "one_slot"])
def test_env_steps_after_a_rollout_keep_the_fallback(device, ring):
    """The rollout turns the step's fallback pass off for its own launches only: 20 direct steps of agent.vec after
    it (every env ends an episode twice, max_steps 12) meet no MERLIN_DEVERR_SLOT_EMPTY."""
    agent = _agent(device, ring)
    for _ in range(2):  # eager + capture, then a replay
        agent.collect_rollouts()
    env = agent.vec
    assert env.step_fallback
    acts = torch.from_numpy(np.random.RandomState(3).randint(0, 3, size=(20, PN)).astype(np.int64)).to(device)
    done = torch.zeros((20, PN), dtype=torch.float32, device=device)
    for t in range(20):
        env.step_into(acts[t], None, None, None, None, done[t])
    flags, _ = env.errors(raise_on_error=False)
    assert flags == 0
    assert (done.sum(0) >= 1).all()
    agent.collect_rollouts()  # and the next rollout finds its rings topped up in-stream
    env.errors()
