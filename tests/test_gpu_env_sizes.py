"""GPU parity: the HIP env kernels against the C oracle over the grid sizes, bit-exact.

tests/test_gpu_env.py runs 16x16 (and 22x22); the kernels' behaviour depends on the size in more places than that:
the two row-store instantiations (SP = 16 up to size 16, SP = 32 above) with padded rows below 16 and at 17..31 and
with bit 31 the border wall at 32, gen_hard's small-grid generator (size <= 10), gen_mediumhard's wall count, the
default episode length 4 * size^2, and the goal of `easy` at size 5, which replaces the border wall's corner.  The
oracle itself is pinned to the literal MiniGrid model at every size in tests/test_oracle_sizes.py.

n = 300 envs everywhere: the last step block (128 envs) and the last reset block (64) are partial."""
import ctypes as C

import numpy as np
import pytest
import torch

from minigrid_literal import LiteralEnv

pytestmark = pytest.mark.gpu

N = 300
P_FWD = [0.15, 0.15, 0.7]  # forward-biased, as test_gpu_env.test_large_batch_vs_oracle


def unpack(codes_i32: torch.Tensor) -> np.ndarray:
    """int32[..., 8] nibble words -> uint8[..., 49] tile classes."""
    w = codes_i32.cpu().numpy().astype(np.uint32).view(np.uint32)
    nib = (w[..., :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xF
    return nib.reshape(*w.shape[:-1], 64)[..., :49].astype(np.uint8)


def make_env(n, diff, size, seed, device, **kw):
    from merlin import MerlinVecEnv

    return MerlinVecEnv(n, difficulty=diff, size=size, seed=seed, device=device, **kw)


def seeds_of(base, n=N):
    return np.arange(base, base + n, dtype=np.uint64)


def actions(seed, T, p=P_FWD, n=N):
    return np.random.RandomState(seed).choice([0, 1, 2], size=(T, n), p=p).astype(np.int64)


def single_steps(env, acts, device):
    """T single-step launches; everything a step writes, on the host."""
    T, n = acts.shape
    codes = torch.zeros((T, n, 8), dtype=torch.int32, device=device)
    rew = torch.zeros((T, n), dtype=torch.float32, device=device)
    term = torch.zeros((T, n), dtype=torch.uint8, device=device)
    trunc = torch.zeros((T, n), dtype=torch.uint8, device=device)
    done = torch.zeros((T, n), dtype=torch.float32, device=device)
    ta = torch.from_numpy(acts).to(device)
    for t in range(T):
        env.step_into(ta[t], codes[t], rew[t], term[t], trunc[t], done[t])
    return unpack(codes), rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), done.cpu().numpy()


def assert_maps(oracle, st, diff, size, seeds):
    """The state a seeded reset left against oracle.gen_map of each env's seed."""
    for i, s in enumerate(seeds):
        cells, meta = oracle.gen_map(size, diff, int(s))
        assert (st["cells"][i] == cells).all(), (size, i)
        assert tuple(st["agent_pos"][i]) == tuple(meta[0:2]) and st["agent_dir"][i] == meta[2], (size, i)
        assert tuple(st["goal_pos"][i]) == tuple(meta[3:5]), (size, i)


def no_errors(env):
    flags, _ = env.errors()
    assert flags == 0


# difficulty -> sizes; (difficulty, size) -> (max_steps, T) where not (40, 120).  None: the default 4 * size^2.
MATRIX = {
    "easy": [5, 6, 17, 32],
    "medium": [5, 15, 17, 32],
    "mediumhard": [5, 6, 15, 17, 31, 32],
    "hard": [5, 6, 10, 11, 17, 31, 32],
    "hardest": [8, 9, 15, 17, 32],
}
EPISODE = {("mediumhard", 5): (None, 120), ("hard", 6): (30, 120), ("easy", 32): (60, 120), ("easy", 17): (60, 120),
           ("hard", 5): (30, 120), ("easy", 5): (40, 96)}
# no termination expected from random actions: the goal is behind a wall with 2..5 one-cell gaps, 15 columns away
TRUNC_ONLY = {("hard", 31), ("hard", 32)}
CASES = [(d, s) for d, sizes in MATRIX.items() for s in sizes]


@pytest.mark.parametrize("diff,size", CASES, ids=[f"{d}-{s}" for d, s in CASES])
def test_rollout_vs_oracle(oracle, device, diff, size):
    """Seeded reset, then T single-step launches with auto-reset, every env and step against the oracle: the reset
    observation, each step's codes / reward / term / trunc / done, the final agent state, and the maps of the seeded
    reset.  The oracle's own rollout must hold truncations and terminations, so nothing passes vacuously -- except
    `hard` at 31 and 32 (truncations only: random actions do not find the gaps of a wall 15 columns from the goal;
    the CPU run shows none) and `easy` at 5, where the goal is the border's corner (0, 0) and can never be entered:
    there the goal tile must show in more than a quarter of the oracle's frames."""
    max_steps, T = EPISODE.get((diff, size), (40, 120))
    base = 777 + 1000 * size
    acts = actions(size, T)
    env = make_env(N, diff, size, base, device, max_steps=max_steps)
    obs0 = unpack(env.reset().clone())
    assert_maps(oracle, env.get_state(), diff, size, seeds_of(base))
    codes, rew, term, trunc, done = single_steps(env, acts, device)
    ocodes, orew, oterm, otrunc, oagent = oracle.batch_rollout(seeds_of(base), acts, size=size, difficulty=diff,
                                                               max_steps=max_steps or 0)
    assert otrunc.sum() > 0
    if (diff, size) == ("easy", 5):
        assert oterm.sum() == 0 and (ocodes == 3).any(-1).mean() > 0.25
    elif (diff, size) not in TRUNC_ONLY:
        assert oterm.sum() > 0
    assert (obs0 == ocodes[0]).all()
    assert (codes == ocodes[1:]).all()
    assert (rew == orew).all()
    assert (term == oterm).all() and (trunc == otrunc).all()
    assert (done == np.maximum(oterm, otrunc)).all()
    st = env.get_state()
    assert (st["agent_pos"] == oagent[-1][:, 0:2]).all() and (st["agent_dir"] == oagent[-1][:, 2]).all()
    assert (st["step_count"] == oagent[-1][:, 3]).all()
    no_errors(env)


@pytest.mark.parametrize("diff", list(MATRIX))
def test_seeded_maps_at_every_size(oracle, device, diff):
    """Map generation alone at every size 5..32 (hardest: 8..32): 70 envs (a partial second reset block) against
    oracle.gen_map.  gen_mediumhard's wall count int(playable * 0.10) .. int(playable * 0.20) is integer arithmetic
    in the kernel and floating point in the reference: every value of playable = (size - 2)^2 is here."""
    for size in range(8 if diff == "hardest" else 5, 33):
        env = make_env(70, diff, size, 31 * size, device)
        env.reset()
        assert_maps(oracle, env.get_state(), diff, size, seeds_of(31 * size, 70))
        no_errors(env)
        env.close()


@pytest.mark.parametrize("diff", list(MATRIX))
def test_short_rollout_at_every_size(oracle, device, diff):
    """48 steps with episodes of at most 12 at every size 5..32 (hardest: 8..32): the view's window over padded rows
    (the out-of-grid mask starts at bit size + 8) and the resets' look-ahead slots at each row count, against the
    oracle.  The longer runs with their coverage conditions are test_rollout_vs_oracle's."""
    T, max_steps = 48, 12
    for size in range(8 if diff == "hardest" else 5, 33):
        base = 13 * size
        acts = actions(100 + size, T)
        env = make_env(N, diff, size, base, device, max_steps=max_steps)
        obs0 = unpack(env.reset().clone())
        codes, rew, term, trunc, done = single_steps(env, acts, device)
        ocodes, orew, oterm, otrunc, oagent = oracle.batch_rollout(seeds_of(base), acts, size=size, difficulty=diff,
                                                                   max_steps=max_steps)
        assert otrunc.sum() > N, size
        assert (obs0 == ocodes[0]).all() and (codes == ocodes[1:]).all(), size
        assert (rew == orew).all() and (term == oterm).all() and (trunc == otrunc).all(), size
        assert (done == np.maximum(oterm, otrunc)).all(), size
        st = env.get_state()
        assert (st["agent_pos"] == oagent[-1][:, 0:2]).all() and (st["agent_dir"] == oagent[-1][:, 2]).all(), size
        no_errors(env)
        env.close()


@pytest.mark.parametrize("size", [5, 6])
def test_default_max_steps(oracle, device, size):
    """max_steps not given is 4 * size^2 (100, 144).  Odd envs only turn: truncated exactly at the default, not
    before; even envs walk: the reward 1 - 0.9 * steps / max_steps of the goals they reach uses the default."""
    default = 4 * size * size
    T = default + 10
    acts = actions(size, T)
    acts[:, 1::2] = np.random.RandomState(size + 1).randint(0, 2, size=(T, N // 2))
    env = make_env(N, "mediumhard", size, 90 + size, device)
    assert env.max_steps == default
    env.reset()
    codes, rew, term, trunc, done = single_steps(env, acts, device)
    ocodes, orew, oterm, otrunc, _ = oracle.batch_rollout(seeds_of(90 + size), acts, size=size,
                                                          difficulty="mediumhard", max_steps=0)
    assert (otrunc[default - 1, 1::2] == 1).all() and otrunc[:default - 1, 1::2].sum() == 0
    assert oterm.sum() > 0 and len(np.unique(orew[oterm == 1])) > 10
    assert (trunc == otrunc).all() and (term == oterm).all()
    assert (rew == orew).all()
    assert (codes == ocodes[1:]).all()
    no_errors(env)


@pytest.mark.parametrize("diff,size", [("mediumhard", 5), ("hard", 17), ("hardest", 32)])
def test_multistep_launch_vs_oracle(oracle, device, diff, size):
    """n_steps = T in one launch: the state stays on chip and the maps of all resets after an env's first are
    generated inside the launch (max_steps 12: each env resets about eight times)."""
    T, max_steps, base = 96, 12, 4000 + size
    acts = actions(size + 3, T)
    env = make_env(N, diff, size, base, device, max_steps=max_steps)
    env.reset()
    codes = torch.zeros((T, N, 8), dtype=torch.int32, device=device)
    rew = torch.zeros((T, N), dtype=torch.float32, device=device)
    term = torch.zeros((T, N), dtype=torch.uint8, device=device)
    trunc = torch.zeros((T, N), dtype=torch.uint8, device=device)
    env.step_into(torch.from_numpy(acts).to(device), codes, rew, term, trunc, None, n_steps=T, action_stride=N)
    ocodes, orew, oterm, otrunc, oagent = oracle.batch_rollout(seeds_of(base), acts, size=size, difficulty=diff,
                                                               max_steps=max_steps)
    assert otrunc.sum() > 4 * N
    assert (unpack(codes) == ocodes[1:]).all()
    assert (rew.cpu().numpy() == orew).all()
    assert (term.cpu().numpy() == oterm).all() and (trunc.cpu().numpy() == otrunc).all()
    st = env.get_state()
    assert (st["agent_pos"] == oagent[-1][:, 0:2]).all() and (st["agent_dir"] == oagent[-1][:, 2]).all()
    assert (st["step_count"] == oagent[-1][:, 3]).all()
    no_errors(env)


@pytest.mark.parametrize("mode", ["never", "side_stream_every_step"])
@pytest.mark.parametrize("size", [5, 32])
def test_refill_modes_vs_oracle(oracle, device, size, mode):
    """test_gpu_env.test_lookahead_refill_modes_vs_oracle at the edge sizes: no refills at all (every reset after an
    env's first generates in k_env_fallback) and a refill on a side stream after every step."""
    T, max_steps, base = 64, 6, 4242
    acts = actions(5, T, p=[0.1, 0.1, 0.8])
    env = make_env(N, "mediumhard", size, base, device, max_steps=max_steps)
    env.set_refill_interval(0)
    env.reset()
    codes = torch.zeros((T, N, 8), dtype=torch.int32, device=device)
    rew = torch.zeros((T, N), dtype=torch.float32, device=device)
    done = torch.zeros((T, N), dtype=torch.float32, device=device)
    ta = torch.from_numpy(acts).to(device)
    main, side = torch.cuda.current_stream(device), torch.cuda.Stream(device)
    for t in range(T):
        if mode == "side_stream_every_step" and t > 0:
            main.wait_stream(side)
        env.step_into(ta[t], codes[t], rew[t], None, None, done[t])
        if mode == "side_stream_every_step":
            side.wait_stream(main)
            with torch.cuda.stream(side):
                env.refill()
    main.wait_stream(side)
    torch.cuda.synchronize(device)
    ocodes, orew, oterm, otrunc, _ = oracle.batch_rollout(seeds_of(base), acts, size=size, difficulty="mediumhard",
                                                          max_steps=max_steps)
    # several resets of one env inside 16 steps: without refills the fallback path ran
    assert (np.maximum(oterm, otrunc)[:16].sum(0) >= 2).sum() > N // 2
    assert (unpack(codes) == ocodes[1:]).all()
    assert (rew.cpu().numpy() == orew).all()
    assert (done.cpu().numpy() == np.maximum(oterm, otrunc)).all()
    no_errors(env)


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("max_stay,penalty", [(3, -0.1), (1, -0.25), (5, -0.1)])
@pytest.mark.parametrize("size", [5, 32])
def test_wrapper_options_vs_oracle(oracle, device, size, max_stay, penalty, explore):
    """The stuck penalty with max_stay / penalty other than the defaults, with and without the exploration bonus
    (visited bit rows: bit 31 at size 32 is never entered, bit 30 is), rewards exact."""
    T, max_steps, base = 120, 50, 31
    acts = actions(1 + size, T, p=[0.3, 0.3, 0.4])
    env = make_env(N, "mediumhard", size, base, device, max_steps=max_steps, stuck_penalty=True, max_stay=max_stay,
                   penalty=penalty, exploration_bonus=explore, bonus=0.05)
    env.reset()
    codes, rew, term, trunc, done = single_steps(env, acts, device)
    ocodes, orew, oterm, otrunc, _ = oracle.batch_rollout(seeds_of(base), acts, size=size, difficulty="mediumhard",
                                                          max_steps=max_steps, stuck=True, max_stay=max_stay,
                                                          penalty=penalty, explore=explore, explore_bonus=0.05)
    plain = oracle.batch_rollout(seeds_of(base), acts, size=size, difficulty="mediumhard", max_steps=max_steps)[1]
    assert (orew < plain).any() and (orew > plain).any() == explore
    assert (rew == orew).all()
    assert (codes == ocodes[1:]).all() and (term == oterm).all() and (trunc == otrunc).all()
    no_errors(env)


@pytest.mark.parametrize("diff,size", [("hard", 6), ("hardest", 32)])
def test_reseed_each_reset(oracle, device, diff, size):
    """reseed_each_reset: every reset is reset(seed=the env's seed).  Through 63 steps of episodes at most 7 long
    every observation after an episode end is the first one again; afterwards the walls are still the seed's map,
    and an explicit reset gives its agent and direction again."""
    T, max_steps = 63, 7
    seeds = seeds_of(500 + size)
    env = make_env(N, diff, size, None, device, seeds=seeds, reseed_each_reset=True, max_steps=max_steps)
    obs0 = unpack(env.reset().clone())
    assert_maps(oracle, env.get_state(), diff, size, seeds)
    codes, rew, term, trunc, done = single_steps(env, actions(size, T), device)
    assert trunc.sum() > 3 * N
    ends = done > 0
    assert (codes[ends] == np.broadcast_to(obs0, codes.shape)[ends]).all()
    st = env.get_state()
    for i, s in enumerate(seeds):
        cells, meta = oracle.gen_map(size, diff, int(s))
        assert ((st["cells"][i] == 1) == (cells == 1)).all() and tuple(st["goal_pos"][i]) == tuple(meta[3:5])
    assert (unpack(env.reset()) == obs0).all()
    assert_maps(oracle, env.get_state(), diff, size, seeds)
    no_errors(env)


def test_masked_reset_at_32(oracle, device):
    """Masked reset with the 32-row store: unmasked envs keep their walls and observation rows, masked ones take the
    next map of their stream -- the oracle's observation and agent after one truncated step (max_steps 1), and the
    literal model's cells after a second, unseeded reset."""
    size, base = 32, 9
    env = make_env(N, "mediumhard", size, base, device)
    first = env.reset().clone()
    st0 = env.get_state()
    mask = torch.zeros(N, dtype=torch.uint8, device=device)
    mask[::3] = 1
    out = env.reset(mask=mask).clone()
    st1 = env.get_state()
    m = mask.cpu().numpy() > 0
    assert torch.equal(out[mask == 0], first[mask == 0])
    for k in ("walls", "agent_pos", "agent_dir", "goal_pos"):
        assert (st1[k][~m] == st0[k][~m]).all(), k
    ocodes, _, _, otrunc, oagent = oracle.batch_rollout(seeds_of(base), np.zeros((1, N), np.int64), size=size,
                                                        difficulty="mediumhard", max_steps=1)
    assert otrunc.all()
    assert (unpack(out)[m] == ocodes[1][m]).all()
    assert (st1["agent_pos"][m] == oagent[1][m, 0:2]).all() and (st1["agent_dir"][m] == oagent[1][m, 2]).all()
    assert (st1["step_count"][m] == 0).all()
    for i in np.flatnonzero(m)[::5]:
        lit = LiteralEnv(size, "mediumhard")
        lit.reset(seed=base + int(i))
        lit.reset()
        assert (st1["cells"][i] == lit.cells()).all(), i
    no_errors(env)


@pytest.mark.parametrize("diff,size", [("easy", 5), ("hard", 17), ("hardest", 32)])
def test_full_observation_vs_literal(device, diff, size):
    """render_full() after a seeded reset against the literal model's own reset(seed) and full_obs(): independent of
    the state the env reports.  At easy 5 the goal (8, 1, 0) sits where the border's corner was."""
    base = 11
    env = make_env(N, diff, size, base, device)
    env.reset()
    full = env.render_full().cpu().numpy()
    assert full.shape == (N, size, size, 3)
    for i in range(N):
        lit = LiteralEnv(size, diff)
        lit.reset(seed=base + i)
        assert np.array_equal(full[i], lit.full_obs()), i
    if (diff, size) == ("easy", 5):
        assert (full[:, 0, 0] == (8, 1, 0)).all()
    no_errors(env)


def test_create_size_bounds(oracle, device):
    """merlin_env_create follows the reference's generators: sizes 5..32 (32: the width of the bit rows), hardest
    from 8 (tests/test_oracle_sizes.py::test_where_generators_stop), hard from 5."""
    from merlin import _native as nat

    L = nat.lib()
    h = C.c_void_p()
    for size, diff in [(4, "mediumhard"), (33, "mediumhard"), (7, "hardest"), (5, "hardest"), (4, "hard")]:
        cfg = nat.EnvConfig(8, size, nat.DIFFICULTY_IDS[diff], 0, 0, 3, -0.1, 0, 0.0, 0)
        assert L.merlin_env_create(C.byref(cfg), C.byref(h)) == 4, (size, diff)  # MERLIN_E_UNSUPPORTED
        assert not h.value
    for size, diff in [(5, "hard"), (8, "hardest")]:
        env = make_env(8, diff, size, 3, device)
        env.reset()
        assert_maps(oracle, env.get_state(), diff, size, seeds_of(3, 8))
        no_errors(env)
