"""GPU: finite level sets (merlin_env_set_levels) and what is built on them, against tests/level_ref.py and the oracle.

Bank      a seed-built LevelSet equals the oracle's maps for those seeds (sizes 8, 16, 22: both row widths; one
          mixed-difficulty set).
Stepping  N = 130 envs (a partial 128-env step block, a partial wave), max_steps = 5, 40 random steps: every env resets
          at least 8 times.  The expected trajectory is put together on the CPU from the restated draws and the
          oracle's episodes of the drawn levels' seeds (expected()); after every step -- every launch of the
          multi-step kernel -- each env's map, pose and current level equal the bank's entry, its observation the
          oracle's, and the level the step logs for each env (merlin_env_set_level_log) is the one
          it acted in.  Through the multi-step kernel, the single step with and without the fallback pass and the fused
          act + step, at look-ahead depth 1 and 3 and refill interval 0 and 16, with the wrappers' shaping on.
Isolation the envs' RNG streams and look-ahead maps are untouched by level mode.
Weights   a one-hot CDF; a captured step graph draws from a CDF set after the capture.
Scores    the kernel equals the restatement exactly, on both of its paths.
Trainer   PPO on a level set with prioritized replay: the logged levels, the scores and the CDF against the
          restatement, and the rollout graph against eager rollouts bit for bit.
"""
import numpy as np
import pytest
import torch

import level_ref as R
from pathing_ref import oracle_maps

pytestmark = pytest.mark.gpu

N, T, MAX_STEPS, L = 130, 40, 5, 5
LEVEL_SEEDS = [9100 + 7 * l for l in range(L)]
BASE = 4242  # the envs' own seeds: never used by level mode
DIFF_OF = {8: "mediumhard", 16: "mediumhard", 22: "hard"}
MIXED = ["easy", "medium", "mediumhard", "hard", "hardest"]
UNIFORM = np.arange(1, L + 1, dtype=np.float64) / L
FAR = (1 << 32) - 60  # an env_offset that puts the global env indices across 2^32


def unpack(codes_i32: torch.Tensor) -> np.ndarray:
    """int32[..., 8] nibble words -> uint8[..., 49] tile classes."""
    w = codes_i32.cpu().numpy().astype(np.uint32).view(np.uint32)
    nib = (w[..., :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xF
    return nib.reshape(*w.shape[:-1], 64)[..., :49].astype(np.uint8)


def actions():
    return np.random.RandomState(5).randint(0, 3, size=(T, N)).astype(np.int64)


def pick_level_seed(env_offset=0):
    """The first seed under which the restated draws of the first 9 maps of the N envs use all 5 levels."""
    for s in range(100):
        if len(np.unique(R.draws(s, env_offset, N, 0, 9, UNIFORM))) == L:
            return s
    raise AssertionError("no level seed draws every level")


_BANK, _REF = {}, {}


def bank(oracle, size, names=None):
    """(walls uint32[L, S], goal int32[L, 2], agent int32[L, 4]) of the oracle's maps for LEVEL_SEEDS."""
    names = tuple(names or [DIFF_OF[size]] * L)
    if (size, names) not in _BANK:
        parts = [oracle_maps(oracle, d, size, [s])[1:] for d, s in zip(names, LEVEL_SEEDS)]
        out = tuple(np.concatenate([p[j] for p in parts]) for j in range(3))
        for a in out:
            a.setflags(write=False)
        _BANK[(size, names)] = out
    return _BANK[(size, names)]


def expected(oracle, size, level_seed, env_offset=0, shaping=False, cdf=UNIFORM):
    """The trajectory level mode must produce, episode by episode: round k plays every env's k-th map, the level
    level_ref draws for (level_seed, env_offset + i, k), as the oracle plays that level's seed under the env's next
    actions.  Returns codes uint8[T + 1, N, 49], reward, done float32[T, N], level int64[T + 1, N], pose int32[T + 1,
    N, 3] (index t: before step t).  Computed once per case and never modified."""
    key = (size, level_seed, env_offset, shaping, tuple(cdf))
    if key in _REF:
        return _REF[key]
    acts = actions()
    codes = np.zeros((T + 1, N, 49), dtype=np.uint8)
    rew = np.zeros((T, N), dtype=np.float32)
    done = np.zeros((T, N), dtype=np.float32)
    level = np.full((T + 1, N), -1, dtype=np.int64)
    pose = np.zeros((T + 1, N, 3), dtype=np.int32)
    t0 = np.zeros(N, dtype=np.int64)
    env = np.array([(env_offset + i) & ((1 << 64) - 1) for i in range(N)], dtype=np.uint64)
    k = 0
    while (t0 <= T).any():
        lv = R.draw(level_seed, env, np.uint64(k), cdf)
        a_k = np.zeros((MAX_STEPS, N), dtype=np.int64)
        for s in range(MAX_STEPS):
            tt = np.minimum(t0 + s, T - 1)
            a_k[s] = np.where(t0 + s < T, acts[tt, np.arange(N)], 0)
        oc, orew, ote, otr, oag = oracle.batch_rollout(np.array(LEVEL_SEEDS, dtype=np.uint64)[lv], a_k, size=size,
                                                       difficulty=DIFF_OF[size], max_steps=MAX_STEPS, stuck=shaping,
                                                       explore=shaping, explore_bonus=0.01)
        od = np.maximum(ote, otr)
        assert od.any(0).all()  # max_steps ends every episode inside the window
        length = od.argmax(0) + 1
        for i in np.flatnonzero(t0 <= T):
            b = int(t0[i])
            codes[b, i], level[b, i], pose[b, i] = oc[0, i], lv[i], oag[0, i, :3]
            for s in range(int(length[i])):
                if b + s >= T:
                    break
                rew[b + s, i], done[b + s, i] = orew[s, i], od[s, i]
                if s < length[i] - 1:
                    codes[b + s + 1, i], level[b + s + 1, i], pose[b + s + 1, i] = oc[s + 1, i], lv[i], oag[s + 1, i, :3]
            t0[i] += length[i]
        k += 1
    assert (level >= 0).all() and (done.sum(0) >= 8).all() and k >= 9
    assert len(np.unique(level)) == L  # every level is played
    out = (acts, codes, rew, done, level, pose)
    for a in out:
        a.setflags(write=False)
    _REF[key] = out
    return out


def level_set(device, size, names=None):
    from merlin.levels import LevelSet

    return LevelSet.from_seeds(LEVEL_SEEDS, difficulties=list(names or [DIFF_OF[size]] * L), size=size, device=device)


def make_env(device, size, depth=1, refill=16, env_offset=0, shaping=False, max_steps=MAX_STEPS, n=N):
    from merlin import MerlinVecEnv

    env = MerlinVecEnv(n, difficulty=DIFF_OF[size], size=size, seed=BASE, device=device, max_steps=max_steps,
                       env_offset=env_offset, stuck_penalty=shaping, exploration_bonus=shaping, bonus=0.01)
    env.set_refill_interval(refill)
    if depth != 1:
        env.set_lookahead_depth(depth)
    return env


def state_of(env):
    """(walls, goal, pose, level) of every env now, on the device."""
    walls, goal, agent = env.snapshot()
    return walls, goal, agent[:, :3].clone(), env.current_levels()


def run(env, acts, device, path):
    """reset, then T auto-resetting steps along `path`; (codes [T + 1], reward, done) and {t: state before step t}
    for every t at which the path returns to the host (every step; every 8th for the multi-step kernel)."""
    codes = torch.zeros((T + 1, N, 8), dtype=torch.int32, device=device)
    rew = torch.zeros((T, N), dtype=torch.float32, device=device)
    done = torch.zeros((T, N), dtype=torch.float32, device=device)
    ta = torch.from_numpy(acts.copy()).to(device)
    log = torch.full((T, N), -7, dtype=torch.int32, device=device)  # the step's own log of the levels acted in
    env.reset(out=codes[0])
    states = {0: state_of(env)}
    if path == "single_nofallback":
        env.set_step_fallback(False)
    if path == "multi":
        for t in range(0, T, 8):
            env.set_level_log(log[t:t + 8])
            env.step_into(ta[t:t + 8], codes[t + 1:t + 9], rew[t:t + 8], None, None, done[t:t + 8], n_steps=8,
                          action_stride=N)
            states[t + 8] = state_of(env)
    elif path == "fused":
        ba = torch.zeros(3, device=device)
        bc = torch.zeros(1, device=device)
        out = tuple(torch.empty(N, dtype=dt, device=device) for dt in (torch.int64, torch.float32, torch.float32))
        for t in range(T):
            part = torch.zeros((2, 1, N, 4), device=device)
            part[0, 0, torch.arange(N, device=device), ta[t]] = 5.0  # the argmax is the scripted action
            env.set_level_log(log[t])
            env.act_step_into(part, ba, bc, out, codes[t + 1], rew[t], None, None, done[t], deterministic=True)
            assert torch.equal(out[0], ta[t])
            states[t + 1] = state_of(env)
    else:
        for t in range(T):
            env.set_level_log(log[t])
            env.step_into(ta[t], codes[t + 1], rew[t], None, None, done[t])
            states[t + 1] = state_of(env)
    env.set_level_log(None)
    return unpack(codes), rew.cpu().numpy(), done.cpu().numpy(), states, log.cpu().numpy()


def check(got, ref, bk):
    codes, rew, done, states, log = got
    _, ocodes, orew, odone, olevel, opose = ref
    assert (log == olevel[:T]).all()
    assert (codes == ocodes).all()
    assert (rew == orew).all()
    assert (done == odone).all()
    bw, bg, _ = bk
    for t, (walls, goal, pose, level) in states.items():
        lv = level.cpu().numpy().astype(np.int64)
        assert (lv == olevel[t]).all(), t
        assert (walls.cpu().numpy().view(np.uint32) == bw[lv]).all(), t
        assert (goal.cpu().numpy() == bg[lv]).all(), t
        assert (pose.cpu().numpy() == opose[t]).all(), t


def no_errors(env):
    flags, _ = env.errors(raise_on_error=False)
    assert flags == 0  # MERLIN_DEVERR_SLOT_EMPTY among them


# ------------------------------------------------------------------------------------------------------------ bank
@pytest.mark.parametrize("size,names", [(8, None), (16, None), (22, None), (16, MIXED)],
                         ids=["8", "16", "22", "16_mixed"])
def test_seed_built_bank_equals_the_oracles_maps(oracle, device, size, names):
    ls = level_set(device, size, names)
    bw, bg, ba = bank(oracle, size, names)
    assert len(ls) == L and ls.size == size and ls.seeds == LEVEL_SEEDS
    assert (ls.walls.cpu().numpy().view(np.uint32) == bw).all()
    assert (ls.goal.cpu().numpy() == bg).all()
    assert (ls.agent.cpu().numpy() == ba).all()


def test_level_set_from_arrays_and_file_bind_like_the_seed_built_one(oracle, device, tmp_path):
    """The oracle's maps through from_arrays (solvable), saved, loaded and bound: the same resets as the seed-built
    set's."""
    from merlin.levels import LevelSet

    bw, bg, ba = bank(oracle, 16)
    hand = LevelSet.from_arrays(bw, bg, ba, solvable=True)
    hand.save(str(tmp_path / "bank.npz"))
    sets = [level_set(device, 16), LevelSet.load(str(tmp_path / "bank.npz"), device=device)]
    obs = []
    for ls in sets:
        env = make_env(device, 16)
        env.set_levels(ls, 3)
        obs.append(env.reset().clone())
        env.close()
    assert torch.equal(obs[0], obs[1])


# -------------------------------------------------------------------------------------------------------- stepping
PATHS = ["multi", "single", "single_nofallback", "fused"]


@pytest.mark.parametrize("depth,refill", [(1, 16), (3, 0), (1, 0), (3, 16)])
@pytest.mark.parametrize("path", PATHS)
def test_stepping_16(oracle, device, path, depth, refill):
    seed = pick_level_seed()
    ref = expected(oracle, 16, seed)
    env = make_env(device, 16, depth, refill)
    env.set_levels(level_set(device, 16), seed)
    check(run(env, ref[0], device, path), ref, bank(oracle, 16))
    no_errors(env)
    env.close()


@pytest.mark.parametrize("path,depth,refill", [("multi", 3, 0), ("single", 1, 16), ("single_nofallback", 3, 0),
                                                ("fused", 1, 0)])
def test_stepping_22_far_env_offset(oracle, device, path, depth, refill):
    """32 rows per map (128-B fetches), and global env indices across 2^32 in the draw's key."""
    seed = pick_level_seed(FAR)
    ref = expected(oracle, 22, seed, env_offset=FAR)
    env = make_env(device, 22, depth, refill, env_offset=FAR)
    env.set_levels(level_set(device, 22), seed)
    check(run(env, ref[0], device, path), ref, bank(oracle, 22))
    no_errors(env)
    env.close()


@pytest.mark.parametrize("path", PATHS)
def test_stepping_with_stuck_penalty_and_exploration_bonus(oracle, device, path):
    """The wrappers' state (the stay counter, the visited cells) restarts with every fetched level as with every
    generated map."""
    seed = pick_level_seed()
    ref = expected(oracle, 16, seed, shaping=True)
    assert (ref[2] < 0).any() and ((ref[2] > 0) & (ref[3] == 0)).any()  # penalties and bonuses are paid
    env = make_env(device, 16, shaping=True)
    env.set_levels(level_set(device, 16), seed)
    check(run(env, ref[0], device, path), ref, bank(oracle, 16))
    no_errors(env)
    env.close()


def test_masked_reset_draws_for_the_masked_envs_only(oracle, device):
    seed = pick_level_seed()
    env = make_env(device, 16)
    env.set_levels(level_set(device, 16), seed)
    env.reset()
    mask = torch.zeros(N, dtype=torch.uint8, device=device)
    mask[::3] = 1
    env.reset(mask=mask)
    counts = torch.empty(N, dtype=torch.int32, device=device)
    lv = env.current_levels(counts=counts).cpu().numpy()
    m = mask.cpu().numpy().astype(bool)
    assert (counts.cpu().numpy() == 1 + m).all()
    d = R.draws(seed, 0, N, 0, 2, UNIFORM)
    assert (lv == np.where(m, d[:, 1], d[:, 0])).all()
    no_errors(env)
    env.close()


# ------------------------------------------------------------------------------------------------------- isolation
@pytest.mark.parametrize("filled", [False, True], ids=["empty_slots", "filled_slots"])
def test_level_mode_leaves_the_rng_streams_alone(oracle, device, filled):
    """get_state's rng rows before set_levels, after 40 level-mode steps and after the unbinding are the same, and
    the next reset gives the map the env's stream would have given: the first map of seed BASE + i."""
    acts = actions()
    env = make_env(device, 16)
    env.ensure_seeded()
    if filled:
        env.refill()  # the look-ahead slots hold that first map already
    rng0 = env.get_state()["rng"].copy()
    env.set_levels(level_set(device, 16), 1)
    env.reset()
    ta = torch.from_numpy(acts).to(device)
    for t in range(T):
        env.step_into(ta[t], None, None, None, None, None)
    assert (env.get_state()["rng"] == rng0).all()
    env.set_levels(None)
    assert env.num_levels == 0 and (env.get_state()["rng"] == rng0).all()
    oc = oracle.batch_rollout(np.arange(BASE, BASE + N, dtype=np.uint64), np.zeros((1, N), dtype=np.int64), size=16,
                              difficulty=DIFF_OF[16], max_steps=MAX_STEPS)[0]
    assert (unpack(env.reset().clone()) == oc[0]).all()
    no_errors(env)
    env.close()


def test_binding_rules(device):
    from merlin import MerlinVecEnv
    from merlin import _native as nat

    ls = level_set(device, 16)
    env = make_env(device, 16, n=4)
    with pytest.raises(ValueError):
        env.set_level_cdf(torch.ones(L, dtype=torch.float64, device=device))  # nothing bound
    cdf = torch.ones(L, dtype=torch.float64, device=device)
    assert nat.lib().merlin_env_set_level_cdf(env._h, nat.ptr(cdf), env._stream) == nat.E_INVALID
    with pytest.raises(nat.MerlinNativeError) as e:
        env.current_levels()
    assert e.value.code == nat.E_INVALID
    with pytest.raises(nat.MerlinNativeError) as e:
        env.set_level_log(torch.zeros(4, dtype=torch.int32, device=device))
    assert e.value.code == nat.E_INVALID
    env.set_level_log(None)
    with pytest.raises(ValueError):
        make_env(device, 22, n=4).set_levels(ls)  # another grid size
    walls, goal, agent = (t.contiguous() for t in (ls.walls, ls.goal, ls.agent))
    rc = nat.lib().merlin_env_set_levels(env._h, nat.ptr(walls), nat.ptr(goal), nat.ptr(agent), (1 << 20) + 1, 0, 0,
                                         env._stream)
    assert rc == nat.E_INVALID
    rc = nat.lib().merlin_env_set_levels(env._h, nat.ptr(walls), nat.ptr(goal), nat.ptr(agent), -1, 0, 0, env._stream)
    assert rc == nat.E_INVALID
    env.set_levels(ls, 1)
    with pytest.raises(ValueError):
        env.set_level_cdf(torch.ones(L + 1, dtype=torch.float64, device=device))
    env.set_levels(ls, 2)  # binding again replaces the bank and restarts the counters
    env.reset()
    counts = torch.empty(4, dtype=torch.int32, device=device)
    env.current_levels(counts=counts)
    assert counts.tolist() == [1] * 4
    env.close()
    rs = MerlinVecEnv(4, DIFF_OF[16], size=16, seeds=[1, 2, 3, 4], device=device, reseed_each_reset=True)
    with pytest.raises(nat.MerlinNativeError) as e:
        rs.set_levels(ls, 1)
    assert e.value.code == nat.E_UNSUPPORTED
    rs.close()


# --------------------------------------------------------------------------------------------------------- weights
def test_one_hot_cdf_sends_every_reset_to_that_level(oracle, device):
    bw, bg, _ = bank(oracle, 16)
    env = make_env(device, 16)
    env.set_levels(level_set(device, 16), 7)
    env.set_level_cdf(torch.from_numpy(R.cdf_of(np.eye(L)[3])).to(device))
    env.reset()
    ta = torch.from_numpy(actions()).to(device)
    done = torch.zeros((12, N), dtype=torch.float32, device=device)
    for t in range(12):
        env.step_into(ta[t], None, None, None, None, done[t])
        walls, goal, _, level = state_of(env)
        assert (level == 3).all()
        assert (walls.cpu().numpy().view(np.uint32) == bw[3]).all() and (goal.cpu().numpy() == bg[3]).all()
    assert (done.sum(0) >= 2).all()
    no_errors(env)
    env.close()


def test_captured_step_reads_a_cdf_set_after_the_capture(device):
    """max_steps = 1: every step resets every env, so replay r is draw r of every env.  The graph is captured under
    the uniform CDF; later CDFs reach its replays through the context's buffer, without a re-capture."""
    from merlin import _native as nat

    seed = 11
    env = make_env(device, 16, max_steps=1)
    env.set_levels(level_set(device, 16), seed)
    env.reset()  # draw 0
    acts = torch.zeros(N, dtype=torch.int64, device=device)
    done = torch.zeros(N, dtype=torch.float32, device=device)
    level = torch.empty(N, dtype=torch.int32, device=device)
    env.step_into(acts, None, None, None, None, done)  # draw 1, eager (and the capture's warm-up)
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    with nat.capture_guard(), torch.cuda.graph(g):
        env.step_into(acts, None, None, None, None, done)
        env.current_levels(out=level)
    skewed = R.cdf_of([0.3, 0.2, 0.0, 0.1, 0.4])
    k = 2
    for cdf in (UNIFORM, R.cdf_of(np.eye(L)[2]), skewed, UNIFORM):
        env.set_level_cdf(torch.from_numpy(cdf).to(device))
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize(device)
            assert (done == 1).all()
            assert (level.cpu().numpy() == R.draws(seed, 0, N, k, 1, cdf)[:, 0]).all(), k
            k += 1
    no_errors(env)
    env.close()


# ---------------------------------------------------------------------------------------------------------- scores
# (T, N, L): the issue's two shapes; more than one column tile and step slab; the LDS path's last L and the direct
# path's first
SCORE_SHAPES = [(7, 130, 5), (3, 70, 5000), (40, 600, 37), (5, 300, 2048), (5, 300, 2049)]


@pytest.mark.parametrize("T_,N_,L_", SCORE_SHAPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_level_scores_kernel_equals_restatement(device, T_, N_, L_, kind):
    from merlin import _native as nat

    adv, lv = R.score_case(T_, N_, L_, 3)
    rs, rc = R.scores(adv, lv, L_, kind)
    assert (rc == 0).any() and (rc > 0).any()
    d_adv, d_lv = torch.from_numpy(adv).to(device), torch.from_numpy(lv).to(device)
    s, c = nat.level_scores(d_adv, d_lv, L_, kind)
    assert s.dtype == c.dtype == torch.int64
    assert (s.cpu().numpy() == rs).all() and (c.cpu().numpy() == rc).all()
    # accumulate: another rollout added to these; without it the vectors are overwritten
    adv2, lv2 = R.score_case(T_, N_, L_, 4)
    nat.level_scores(torch.from_numpy(adv2).to(device), torch.from_numpy(lv2).to(device), L_, kind, sum=s, count=c,
                     accumulate=True)
    rs2, rc2 = R.scores(adv2, lv2, L_, kind, rs, rc)
    assert (s.cpu().numpy() == rs2).all() and (c.cpu().numpy() == rc2).all()
    nat.level_scores(d_adv, d_lv, L_, "l1_value" if kind == 0 else "positive_value", sum=s, count=c)
    assert (s.cpu().numpy() == rs).all() and (c.cpu().numpy() == rc).all()
    hs, hc = nat.level_scores_host(adv, lv, L_, kind)
    assert (hs == rs).all() and (hc == rc).all()


def test_level_scores_one_level_takes_every_step(device):
    """The worst contention there is: every step of 128 x 512 lands on one address."""
    from merlin import _native as nat

    adv = torch.full((128, 512), 0.75, device=device)
    lv = torch.full((128, 512), 3, dtype=torch.int32, device=device)
    for L_ in (5, 4000):
        s, c = nat.level_scores(adv, lv, L_, 0)
        want = np.zeros(L_, dtype=np.int64)
        want[3] = 128 * 512
        assert (c.cpu().numpy() == want).all() and (s.cpu().numpy() == want * (3 << 22)).all()


# --------------------------------------------------------------------------------------------------------- trainer
PN, PT, PL = 64, 8, 8
P_SEEDS = [700 + l for l in range(PL)]


def _agent(device, graph):
    from merlin import MerlinVecEnv
    from merlin.levels import LevelSampler, LevelSet
    from merlin.ppo import PPO

    ls = LevelSet.from_seeds(P_SEEDS, difficulty="mediumhard", size=16, device=device)
    env = MerlinVecEnv(PN, "mediumhard", seed=777, device=device, max_steps=6)
    torch.manual_seed(0)
    sampler = LevelSampler(PL, "plr", beta=0.3, rho=0.2, device=device)
    return PPO(env, batch_size=PN * PT, minibatch_size=PN * PT // 2, update_epochs=1, ent_coef=0.05, device=device,
               rollout_graph=graph, level_set=ls, level_sampler=sampler, level_seed=5)


def _iterations(device, graph, n=3):
    agent = _agent(device, graph)
    assert not agent._ring and agent.vec.lookahead_depth == 1  # the map ring is off
    out = []
    for _ in range(n):
        lv = agent.collect_rollouts()
        torch.cuda.synchronize(device)
        row = {f: getattr(agent.buf, f).cpu().numpy().copy() for f in ("levels", "actions", "rewards", "dones")}
        agent.update(lv)
        row["adv"] = agent.buf.adv.cpu().numpy().copy()
        row["sum"], row["count"] = (x.cpu().numpy().copy() for x in agent.last_level_scores)
        row["cdf"] = agent.last_level_cdf.cpu().numpy().copy()
        out.append(row)
    assert (agent._graph is not None) == graph
    agent.vec.errors()
    return out


_RUNS = {}


def iterations(device, graph):
    if graph not in _RUNS:
        _RUNS[graph] = _iterations(device, graph)
    return _RUNS[graph]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_trainer_levels_scores_and_cdf_equal_the_restatement(device, graph):
    """Three iterations (eager, then -- with the graph -- two replays).  The level logged at step t is the restated
    draw under the CDF in force (uniform first, then the one the update before handed over), counted on from the
    rollout's top reset by the dones; scores exactly, the CDF within 1e-14 (float64 pow and an 8-term prefix sum on
    the device against numpy's: a few ulps of values <= 1)."""
    rows = iterations(device, graph)
    ref = R.Sampler(PL, "plr", 0.3, 0.2)
    k0 = np.zeros(PN, dtype=np.int64)
    cdf = np.arange(1, PL + 1, dtype=np.float64) / PL
    env = np.arange(PN, dtype=np.uint64)
    for it, row in enumerate(rows, 1):
        done = row["dones"] > 0
        assert done.any(0).all()  # max_steps 6 < 8 steps: every env resets inside the rollout
        before = np.concatenate([np.zeros((1, PN), dtype=np.int64), np.cumsum(done, 0)[:-1]])
        want = R.draw(5, env[None, :], (k0[None, :] + before).astype(np.uint64), cdf)
        assert (row["levels"] == want).all(), it
        k0 += 1 + done.sum(0)
        s, c = R.scores(row["adv"], row["levels"], PL, 0)
        assert (row["sum"] == s).all() and (row["count"] == c).all() and c.sum() == PN * PT
        ref.update(s, c, it)
        assert np.abs(row["cdf"] - ref.cdf()).max() <= 1e-14
        assert (np.diff(row["cdf"]) >= 0).all() and row["cdf"][-1] == 1.0
        cdf = row["cdf"]  # the draws that follow read the device's own CDF
    assert not np.allclose(rows[-1]["cdf"], np.arange(1, PL + 1) / PL)  # replay is prioritized by now


def test_trainer_rollout_graph_equals_eager(device):
    on, off = iterations(device, True), iterations(device, False)
    for k, (a, b) in enumerate(zip(on, off)):
        for f in ("levels", "actions", "rewards", "dones", "sum", "count", "cdf"):
            assert (a[f] == b[f]).all(), (k, f)


def test_ppo_rejects_a_sampler_of_another_length(device):
    from merlin import MerlinVecEnv
    from merlin.levels import LevelSampler, LevelSet
    from merlin.ppo import PPO

    ls = LevelSet.from_seeds(P_SEEDS, difficulty="mediumhard", size=16, device=device)
    env = MerlinVecEnv(PN, "mediumhard", seed=777, device=device, max_steps=6)
    with pytest.raises(ValueError):
        PPO(env, batch_size=PN * PT, minibatch_size=PN * PT, device=device, level_set=ls,
            level_sampler=LevelSampler(PL + 1, device=device))
    with pytest.raises(ValueError):
        PPO(env, batch_size=PN * PT, minibatch_size=PN * PT, device=device,
            level_sampler=LevelSampler(PL, device=device))
    env.close()


# ------------------------------------------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("diff,size", [("mediumhard", 16), ("hard", 22)])
def test_evaluate_levels_equals_evaluate_seeds(device, diff, size):
    from merlin.actor_critic import CNNActorCritic
    from merlin.evaluation import evaluate_levels, evaluate_seeds
    from merlin.levels import LevelSet

    seeds = list(range(31000, 31024))
    torch.manual_seed(size)
    ac = CNNActorCritic((56, 56, 3), 3).to(device)
    ls = LevelSet.from_seeds(seeds, difficulty=diff, size=size, device=device)
    for ms in (None, 40):
        rew, steps = evaluate_seeds(ac, seeds, difficulty=diff, size=size, device=device, max_steps=ms)
        lrew, lsteps = evaluate_levels(ac, ls, device=device, max_steps=ms)
        assert lsteps == [int(s) for s in steps]
        assert (np.asarray(lrew, dtype=np.float32) == np.asarray(rew, dtype=np.float64).astype(np.float32)).all()
