"""CPU: the C oracle pinned to the literal MiniGrid model (oracle/minigrid_literal.py, run on numpy's own Generator)
at every grid size the library accepts, 5..32, for every difficulty whose generator runs at that size -- the recorded
fixtures hold 16x16 and 22x22 only.  Both models live in the repository, so the literal is stepped live: a seeded
reset, then the actions with an unseeded reset after every episode end, as oracle.batch_rollout does.  Every
comparison is exact (maps, agent, goal, observation codes, reward as float32, terminated, truncated, step count).

Also here: the stuck-penalty wrapper with max_stay / penalty other than its defaults against the literal restatement
of it (LiteralStuckPenalty), and the sizes at which the generators stop working -- the ground truth for the sizes
merlin_env_create refuses."""
import numpy as np
import pytest

from minigrid_literal import LiteralEnv, LiteralStuckPenalty

DIFFS = ["easy", "medium", "mediumhard", "hard", "hardest"]
SIZES = list(range(5, 33))
HARDEST_MIN = 8  # hardest_env.py draws integers(2, size // 2 - 1): an empty range below 8 (test_where_generators_stop)

CASES = [(d, s) for d in DIFFS for s in SIZES if d != "hardest" or s >= HARDEST_MIN]


def literal_rollout(size, diff, seeds, acts, max_steps, stuck=None):
    """The literal model through the same schedule as oracle.batch_rollout; also the cells / goal after the seeded
    reset.  stuck = (max_stay, penalty) wraps it in LiteralStuckPenalty."""
    T, n = acts.shape
    codes = np.zeros((T + 1, n, 49), dtype=np.uint8)
    rew = np.zeros((T, n), dtype=np.float32)
    term = np.zeros((T, n), dtype=np.uint8)
    trunc = np.zeros((T, n), dtype=np.uint8)
    agent = np.zeros((T + 1, n, 4), dtype=np.int32)
    cells, goals = [], []
    for i, s in enumerate(seeds):
        env = LiteralEnv(size, diff, max_steps)
        w = LiteralStuckPenalty(env, *stuck) if stuck else env
        codes[0, i] = w.reset(seed=int(s)).reshape(-1)
        agent[0, i] = (*env.agent_pos, env.agent_dir, env.step_count)
        cells.append(env.cells())
        goals.append(tuple(env.goal_pos))
        for t in range(T):
            c, r, te, tr = w.step(int(acts[t, i]))
            rew[t, i] = np.float32(r)
            term[t, i], trunc[t, i] = te, tr
            if te or tr:
                c = w.reset()
            codes[t + 1, i] = c.reshape(-1)
            agent[t + 1, i] = (*env.agent_pos, env.agent_dir, env.step_count)
    return codes, rew, term, trunc, agent, cells, goals


def assert_same(got, want):
    for name, g, w in zip(("codes", "reward", "term", "trunc", "agent"), got, want):
        assert g.dtype == w.dtype and (g == w).all(), name


@pytest.mark.parametrize("diff,size", CASES, ids=[f"{d}-{s}" for d, s in CASES])
def test_oracle_equals_literal(oracle, diff, size):
    """10 envs x 60 steps, max_steps 12 so every env is truncated and regenerated several times; forward-biased
    actions so goals are reached where they can be."""
    n, T, max_steps = 10, 60, 12
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(1000 * size + 97 * DIFFS.index(diff))
    acts = np.random.RandomState(size).choice([0, 1, 2], size=(T, n), p=[0.15, 0.15, 0.7]).astype(np.int64)
    *want, cells, goals = literal_rollout(size, diff, seeds, acts, max_steps)
    for i, s in enumerate(seeds):
        c, m = oracle.gen_map(size, diff, int(s))
        assert (c == cells[i]).all(), int(s)
        assert tuple(m[:3]) == tuple(want[4][0, i, :3]) and tuple(m[3:5]) == goals[i], int(s)
    got = oracle.batch_rollout(seeds, acts, size=size, difficulty=diff, max_steps=max_steps)
    assert got[3].sum() > 0  # truncations (and re-generations) happened
    assert_same(got, want)


@pytest.mark.parametrize("diff", ["easy", "mediumhard"])
@pytest.mark.parametrize("size", [5, 6])
def test_default_max_steps(oracle, diff, size):
    """max_steps not given is 4 * size^2 (base_env.py:32-33): 100 and 144.  Odd envs only turn, so they are truncated
    exactly at the default; even envs walk, so a goal's reward 1 - 0.9 * steps / max_steps uses it too."""
    n, T, default = 8, 4 * size * size + 10, 4 * size * size
    rs = np.random.RandomState(size)
    acts = rs.choice([0, 1, 2], size=(T, n), p=[0.15, 0.15, 0.7]).astype(np.int64)
    acts[:, 1::2] = rs.randint(0, 2, size=(T, n // 2))
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(50 + size)
    *want, _, _ = literal_rollout(size, diff, seeds, acts, None)
    got = oracle.batch_rollout(seeds, acts, size=size, difficulty=diff, max_steps=0)
    trunc = got[3]
    assert (trunc[default - 1, 1::2] == 1).all() and trunc[: default - 1, 1::2].sum() == 0
    if (diff, size) != ("easy", 5):  # there the goal is the wall's corner: never reached
        assert got[2].sum() > 0
    assert_same(got, want)


@pytest.mark.parametrize("max_stay,penalty", [(3, -0.1), (1, -0.25), (5, -0.1)])
@pytest.mark.parametrize("size", [5, 16, 32])
def test_stuck_penalty_equals_literal(oracle, size, max_stay, penalty):
    """The oracle's stuck-penalty wrapper against LiteralStuckPenalty; as many turns as forward moves, so the counter
    reaches every max_stay, is cleared by moves, and restarts at the resets (max_steps 20)."""
    n, T, max_steps = 10, 60, 20
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(7 * size)
    acts = np.random.RandomState(size + max_stay).choice([0, 1, 2], size=(T, n), p=[0.3, 0.3, 0.4]).astype(np.int64)
    *want, _, _ = literal_rollout(size, "mediumhard", seeds, acts, max_steps, stuck=(max_stay, penalty))
    got = oracle.batch_rollout(seeds, acts, size=size, difficulty="mediumhard", max_steps=max_steps, stuck=True,
                               max_stay=max_stay, penalty=penalty)
    assert (got[1] == np.float32(penalty)).any() and got[3].sum() > 0
    assert_same(got, want)
    plain = oracle.batch_rollout(seeds, acts, size=size, difficulty="mediumhard", max_steps=max_steps)
    assert (plain[1] >= 0).all()  # off by default


def test_stuck_penalty_defaults_unchanged(oracle):
    """batch_rollout(stuck=True) without the new arguments is StuckPenaltyWrapper's (3, -0.1)."""
    seeds = np.arange(4, dtype=np.uint64)
    acts = np.random.RandomState(0).choice([0, 1, 2], size=(40, 4), p=[0.3, 0.3, 0.4]).astype(np.int64)
    a = oracle.batch_rollout(seeds, acts, stuck=True)
    b = oracle.batch_rollout(seeds, acts, stuck=True, max_stay=3, penalty=-0.1)
    assert_same(a, b)
    assert (a[1] < 0).any()


def test_where_generators_stop():
    """hardest draws integers(2, size // 2 - 1) for its first opening: numpy raises below size 8 (an empty range) and
    the generator runs from 8 up; hard runs at 5 (one gap, one free column each for the goal and the agent).  These
    are the sizes merlin_env_create follows."""
    for size in (5, 6, 7):
        with pytest.raises(ValueError):
            LiteralEnv(size, "hardest").reset(seed=0)
    for seed in range(20):
        LiteralEnv(8, "hardest").reset(seed=seed)
        LiteralEnv(5, "hard").reset(seed=seed)
        for diff in ("easy", "medium", "mediumhard"):
            LiteralEnv(5, diff).reset(seed=seed)
