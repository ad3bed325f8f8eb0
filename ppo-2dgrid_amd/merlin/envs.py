"""GPU-resident MERLIN MiniGrid environments backed by libmerlin_hip.so.

``MerlinVecEnv``  N independent envs in HBM; the fast path used by ``merlin.PPO``.
                  Observations are kept as packed 7x7 tile-class codes (int32[N, 8],
                  32 B/env) and expanded to the RGB frame only when a consumer needs it.
``MerlinEnv``     single-env gym-style wrapper (uint8[56, 56, 3] observations), the
                  drop-in for ``ScenarioCreator.create_env`` of the reference
                  (src/scenario_creator/scenario_creator.py:35-57).

Seeding contract (the reference's training env is unseeded, SURVEY TL;DR 5):
env i of a vector env with base seed s is reset with ``reset(seed=s + env_offset + i)``
once (numpy Generator(PCG64(SeedSequence(.))) as gymnasium does), then every later
reset -- explicit or automatic on done -- continues that env's PCG64 stream unseeded.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _native as nat


class Discrete:
    """Minimal stand-in for gymnasium.spaces.Discrete (gymnasium is optional)."""

    def __init__(self, n: int):
        self.n = n
        self.shape = ()
        self.dtype = np.int64

    def sample(self):
        return int(np.random.randint(self.n))


class Box:
    def __init__(self, low, high, shape, dtype):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype


# algorithmic bytes per env-step of k_env_step in the rollout configuration:
# action 8 + agent state r/w 32 + wall rows 64 + episode accumulators r/w 24 + obs codes 32
# + reward 4 + done 4
ENV_STEP_BYTES = 168


def _entropy_seed() -> int:
    return int.from_bytes(os.urandom(8), "little") >> 1


class MerlinVecEnv:
    """N MERLIN envs stepped by HIP kernels.

    Args mirror the reference's env construction (difficulty / size from
    src/config/scenario.yaml, max_steps = 4*size^2 by default, base_env.py:32-33)
    plus the wrapper flags: ``stuck_penalty`` (StuckPenaltyWrapper semantics,
    stuck_penalty_wrapper.py:3-57; unwired in the reference, so off by default)
    and ``exploration_bonus`` (not defined by the reference; +``bonus`` the first
    time a cell is entered in an episode).

    ``difficulty`` is one name for every env, or a sequence of ``num_envs`` names: env i then generates its maps with
    ``difficulties[i]`` (merlin_env_set_difficulties; ``merlin.task_mix.assign`` builds wave-aligned assignments).
    ``difficulty`` reads "mixed" when the envs differ, ``class_ids`` is the per-env MERLIN_* id on the device.
    """

    def __init__(self, num_envs: int, difficulty: str = "mediumhard", size: int = 16,
                 max_steps: int | None = None, seed: int | None = None, device="cuda",
                 stuck_penalty: bool = False, max_stay: int = 3, penalty: float = -0.1,
                 exploration_bonus: bool = False, bonus: float = 0.01, env_offset: int = 0,
                 seeds=None, reseed_each_reset: bool = False, fully_observable: bool = False, flatten: bool = False):
        self.num_envs = int(num_envs)
        names = None if isinstance(difficulty, str) else self._check_names(difficulty)
        if names is None and difficulty not in nat.DIFFICULTY_IDS:
            raise ValueError(f"Unknown difficulty: {difficulty}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.MerlinNativeError("MerlinVecEnv runs on a GPU device (HIP); got " + str(device))
        # a per-env list: the context is created on its lowest class (every size that class runs at), the list set below
        uniform = difficulty if names is None else min(names, key=nat.DIFFICULTY_IDS.__getitem__)
        self.difficulty = uniform
        self.difficulties = [uniform] * self.num_envs
        self.size = int(size)
        self.max_steps = int(max_steps) if max_steps else 4 * self.size * self.size
        self.env_offset = int(env_offset)
        self.action_space = Discrete(3)
        # the observation wrappers of scenario_creator.py:45-53 (observation.fully_observable / flatten): the step
        # always produces the RGB partial view's tile codes; flat_obs() gives the wrapped observation of a batch --
        # the RGB view (56, 56, 3) or the encoded full grid (size, size, 3), flattened to a vector with flatten
        self.fully_observable, self.flatten = bool(fully_observable), bool(flatten)
        shape = (self.size, self.size, 3) if self.fully_observable else (56, 56, 3)
        if self.flatten:
            shape = (int(np.prod(shape)),)
        self.single_observation_space = Box(0, 255, shape, np.uint8)
        self.observation_space = self.single_observation_space
        cfg = nat.EnvConfig(self.num_envs, self.size, nat.DIFFICULTY_IDS[uniform], self.max_steps,
                            int(stuck_penalty), int(max_stay), float(penalty), int(exploration_bonus),
                            float(bonus), int(reseed_each_reset))
        self._lib = nat.lib()
        nat.drain_deferred()  # releases queued by a capture outside capture_guard (merlin._native.defer_release)
        with torch.cuda.device(self.device):
            h = C.c_void_p()
            nat.check(self._lib.merlin_env_create(C.byref(cfg), C.byref(h)), "merlin_env_create")
        self._h = h
        self.lookahead_depth = 1  # set_lookahead_depth
        self.step_fallback = True  # set_step_fallback
        self._topup = None  # the stream a refill(stream=...) not yet joined runs on
        self.level_set = None  # set_levels: the bound bank (None: the envs generate their maps)
        self.num_levels = 0
        self.class_ids = torch.full((self.num_envs,), nat.DIFFICULTY_IDS[uniform], dtype=torch.uint8,
                                    device=self.device)
        # True once classes are assigned: the kernels then read the context's class buffer instead of the uniform id
        # (launches captured into a graph before that keep reading the uniform id)
        self.per_env_classes = False
        self.uniform_difficulty = uniform
        if names is not None:
            self.set_difficulties(names)
        self._seed_pending = seed
        self._seeded_once = False
        if seeds is not None:
            self.seed_each(seeds)
        self.obs = torch.zeros((self.num_envs, nat.OBS_WORDS), dtype=torch.int32, device=self.device)
        # per-step scratch outputs for the gym-style step()
        n = self.num_envs
        self._rew = torch.zeros(n, dtype=torch.float32, device=self.device)
        self._term = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._trunc = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._epr = torch.zeros(n, dtype=torch.float64, device=self.device)
        self._epl = torch.zeros(n, dtype=torch.int32, device=self.device)

    def close(self):
        """Release the env's device state (merlin_env_destroy: hipFree).  While a HIP-graph capture is open
        (e.g. this env dropped by a GC pass inside another agent's capture) the release waits for it to end:
        a hipFree inside a capture invalidates it (merlin._native.capture_guard)."""
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            lib_ = self._lib
            nat.defer_release(lambda: lib_.merlin_env_destroy(h))

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @property
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def seed(self, seed: int) -> None:
        self.join_refill()
        seeds = (np.arange(self.num_envs, dtype=np.uint64) + np.uint64(self.env_offset)
                 + np.uint64(seed))
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_seed(self._h, seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                self.num_envs, self._stream), "merlin_env_seed")
        self._seeded_once = True

    def set_base_seed(self, seed: int) -> None:
        """Seed the next reset() that is given no seed with base `seed` (env i: seed + env_offset + i),
        as the constructor's `seed` does: for callers holding an env from a factory that, like the
        reference's create_env, ignores its seed argument (ppo_train.py's single env)."""
        self._seed_pending = int(seed)
        self._seeded_once = False

    def seed_each(self, seeds) -> None:
        """Seed env i with seeds[i] (e.g. FOMAML task seeds)."""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        assert seeds.shape == (self.num_envs,)
        self.join_refill()
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_seed(self._h, seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                self.num_envs, self._stream), "merlin_env_seed")
        self._seeded_once = True

    def _check_names(self, names) -> list:
        names = [str(d) for d in names]
        if len(names) != self.num_envs:
            raise ValueError(f"difficulty: {len(names)} names for {self.num_envs} envs")
        for d in names:
            if d not in nat.DIFFICULTY_IDS:
                raise ValueError(f"Unknown difficulty: {d}")
        return names

    def set_difficulties(self, names) -> None:
        """Env i generates its maps with names[i] from its next map generation on (merlin_env_set_difficulties): the
        envs keep their current maps and RNG streams, every look-ahead map is dropped.  The classes live in one
        device buffer of the context, so step / reset launches captured into a graph after the first call read a later
        call's classes without a re-capture.  None restores the constructor's uniform difficulty (and unbinds the
        buffer).  Syncs the current stream."""
        self.join_refill()
        if names is None:
            with torch.cuda.device(self.device):
                nat.check(self._lib.merlin_env_set_difficulties(self._h, None, 0, self._stream),
                          "merlin_env_set_difficulties")
            self.per_env_classes = False
            self.difficulty, self.difficulties = self.uniform_difficulty, [self.uniform_difficulty] * self.num_envs
            self.class_ids.fill_(nat.DIFFICULTY_IDS[self.uniform_difficulty])
            return
        names = self._check_names(names)
        self.set_class_ids(np.array([nat.DIFFICULTY_IDS[d] for d in names], dtype=np.int32))

    def set_class_ids(self, ids) -> None:
        """set_difficulties by MERLIN_* id (int32[num_envs]); the library validates the ids."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32))
        self.join_refill()
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_set_difficulties(self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                            int(ids.size), self._stream),
                      "merlin_env_set_difficulties")
        inv = {v: k for k, v in nat.DIFFICULTY_IDS.items()}
        self.difficulties = [inv[int(v)] for v in ids]
        self.difficulty = self.difficulties[0] if len(set(self.difficulties)) == 1 else "mixed"
        self.class_ids.copy_(torch.from_numpy(ids.astype(np.uint8)))
        self.per_env_classes = True

    def ensure_seeded(self) -> None:
        """Seed the envs now if nothing has yet (the constructor's or set_base_seed's seed, else entropy), as the
        first reset() given no seed would: a caller that refills the look-ahead maps before that reset needs the
        seeds in place, since seeding drops every look-ahead map."""
        if not self._seeded_once:
            self.seed(self._seed_pending if self._seed_pending is not None else _entropy_seed())

    def reset(self, seed: int | None = None, mask: torch.Tensor | None = None, out: torch.Tensor | None = None):
        """Reset all envs (or those with mask != 0).  Returns the obs codes int32[N, 8]."""
        self.join_refill()
        if seed is not None:
            self.seed(seed)
        self.ensure_seeded()
        out = self.obs if out is None else out
        if mask is not None:
            mask = mask.to(torch.uint8).contiguous()
            # keep untouched rows of `out` equal to the current obs
            if out.data_ptr() != self.obs.data_ptr():
                out.copy_(self.obs)
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_reset(self._h, nat.ptr(mask), nat.ptr(out), self._stream),
                      "merlin_env_reset")
        if out.data_ptr() != self.obs.data_ptr():
            self.obs.copy_(out)
        return out

    def step_into(self, actions: torch.Tensor, obs_out: torch.Tensor | None = None, reward=None, term=None,
                  trunc=None, done=None, ep_return=None, ep_length=None, n_steps: int = 1,
                  action_stride: int | None = None, autoreset: bool = True) -> None:
        """Low-level step writing straight into caller buffers (rollout storage).

        For n_steps > 1, row t of every output is [t*N:(t+1)*N] and actions are read at
        t*action_stride + i (state stays on chip across the steps)."""
        assert actions.dtype == torch.int64 and actions.is_contiguous()
        stride = self.num_envs if action_stride is None else int(action_stride)
        self.join_refill()
        with torch.cuda.device(self.device), nat.KernelTimer.span("k_env_step", self.num_envs * n_steps * ENV_STEP_BYTES):
            nat.check(self._lib.merlin_env_step(
                self._h, nat.ptr(actions), int(n_steps), stride, nat.ptr(obs_out), nat.ptr(reward),
                nat.ptr(term), nat.ptr(trunc), nat.ptr(done), nat.ptr(ep_return), nat.ptr(ep_length),
                int(bool(autoreset)), self._stream), "merlin_env_step")

    def act_step_into(self, part: torch.Tensor, b_actor: torch.Tensor, b_critic: torch.Tensor, out, obs_out=None,
                      reward=None, term=None, trunc=None, done=None, ep_return=None, ep_length=None,
                      deterministic: bool = False, seed: int = 0, epoch=None, step: int = 0) -> None:
        """act -> step in one launch (merlin_env_act_step): the actions drawn from the acting GEMM's head partials
        part f32[2, P, N, 4] (merlin._native.h3_gemm_nt_heads(partials_only=True)) exactly as merlin._native.act_draw
        draws them, written to out = (action, logp, value), then one auto-reset step into the other buffers."""
        action, logp, value = out
        P = int(part.shape[1])
        A = int(b_actor.numel())
        assert part.dtype == torch.float32 and part.is_contiguous() and part.shape == (2, P, self.num_envs, 4)
        assert action.dtype == torch.int64 and action.numel() == logp.numel() == value.numel() == self.num_envs
        assert b_critic.numel() == 1 and 1 <= A <= 4
        if not deterministic and epoch is None:
            raise ValueError("act_step_into: a sampled action needs an epoch counter tensor (int64[1] on the device)")
        self.join_refill()
        with torch.cuda.device(self.device), nat.KernelTimer.span("k_env_step", self.num_envs * ENV_STEP_BYTES):
            nat.check(self._lib.merlin_env_act_step(
                self._h, nat.ptr(part), P, nat.ptr(b_actor), nat.ptr(b_critic), A, int(bool(deterministic)),
                int(seed) & 0xFFFFFFFFFFFFFFFF, nat.ptr(epoch), int(step), int(self.env_offset), nat.ptr(action),
                nat.ptr(logp), nat.ptr(value), nat.ptr(obs_out), nat.ptr(reward), nat.ptr(term), nat.ptr(trunc),
                nat.ptr(done), nat.ptr(ep_return), nat.ptr(ep_length), self._stream), "merlin_env_act_step")

    # -- finite level sets (merlin/levels.py) --------------------
    def set_levels(self, level_set, level_seed: int = 0) -> None:
        """Bind a merlin.levels.LevelSet: from now on every map an env takes -- reset() and every auto-reset -- is a
        level of the set, drawn from the sampling CDF (uniform until set_level_cdf) by a counter-keyed uniform of
        (level_seed, env_offset + i, the env's map counter): the same levels whichever kernel resets, and under data
        parallelism the draws of one process over the concatenated envs.  The look-ahead ring and the envs' RNG streams
        are neither read nor written.  None unbinds (the streams continue where they were).  Allocates and syncs the
        current stream; a graph captured before it must be captured again (merlin_env_set_levels)."""
        self.join_refill()
        with torch.cuda.device(self.device):
            if level_set is None:
                nat.check(self._lib.merlin_env_set_levels(self._h, None, None, None, 0, 0, 0, self._stream),
                          "merlin_env_set_levels")
                self.level_set, self.num_levels = None, 0
                return
            if level_set.size != self.size:
                raise ValueError(f"a level set of size {level_set.size} on envs of size {self.size}")
            ls = level_set.to(self.device)
            walls, goal, agent = (t.to(torch.int32).contiguous() for t in (ls.walls, ls.goal, ls.agent))
            nat.check(self._lib.merlin_env_set_levels(self._h, nat.ptr(walls), nat.ptr(goal), nat.ptr(agent), len(ls),
                                                      int(level_seed) & 0xFFFFFFFFFFFFFFFF, int(self.env_offset),
                                                      self._stream), "merlin_env_set_levels")
        self.level_set, self.num_levels = ls, len(ls)

    def set_level_cdf(self, cdf: torch.Tensor) -> None:
        """The sampling CDF float64[num_levels] (non-decreasing, last entry 1.0; LevelSampler.cdf()) copied into the
        context's buffer in place, stream-ordered: step launches captured into a graph read the new weights without a
        re-capture (merlin_env_set_level_cdf)."""
        cdf = cdf.to(device=self.device, dtype=torch.float64).contiguous()
        if cdf.numel() != self.num_levels or not self.num_levels:
            raise ValueError(f"set_level_cdf: {cdf.numel()} entries for {self.num_levels} levels")
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_set_level_cdf(self._h, nat.ptr(cdf), self._stream),
                      "merlin_env_set_level_cdf")

    def current_levels(self, out: torch.Tensor | None = None, counts: torch.Tensor | None = None) -> torch.Tensor:
        """int32[N]: the level each env is in, -1 before its first map (merlin_env_levels: one kernel, no host sync,
        capturable).  `counts` (int32[N], optional) receives the maps each env has taken since set_levels."""
        if out is None:
            out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == self.num_envs
        assert counts is None or (counts.dtype == torch.int32 and counts.is_contiguous()
                                  and counts.numel() == self.num_envs)
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_levels(self._h, nat.ptr(out), nat.ptr(counts), self._stream),
                      "merlin_env_levels")
        return out

    def set_level_log(self, log: torch.Tensor | None) -> None:
        """Where the step launches that follow write the level every env acts in: int32[n_steps, N] (one row per step of
        the launch; merlin_env_set_level_log: host state, no launch -- a launch captured into a graph keeps the tensor it
        was captured with).  None: no log."""
        if log is not None:
            assert log.dtype == torch.int32 and log.is_contiguous() and log.numel() % self.num_envs == 0
        nat.check(self._lib.merlin_env_set_level_log(self._h, nat.ptr(log)), "merlin_env_set_level_log")

    # -- level editing (merlin/level_edit.py) --------------------
    def replace_levels(self, slots: torch.Tensor, children) -> None:
        """Child j of `children` (a LevelSet, or (walls int32[C, size], goal int32[C, 2], agent int32[C, 4])) is packed
        into slot slots[j] (int32[C]) of the bound bank, in place and stream-ordered; a slot outside [0, num_levels)
        skips its child; distinct valid slots are the caller's to guarantee.  The bank keeps its addresses: step launches
        captured into a graph play the new maps without a re-capture.  The CDF and the draw counters are untouched.  An
        env inside a replaced slot plays its copy of the old map to the end of its episode; its current level becomes
        -1, and so do the entries of the level log for its remaining steps (merlin_env_replace_levels: no host sync).
        The env's own `level_set` mirror is not touched: LevelSet.replace_ updates it."""
        walls, goal, agent = ((children.walls, children.goal, children.agent) if hasattr(children, "walls")
                              else children)
        Cn = int(slots.numel())
        assert slots.dtype == torch.int32 and walls.dtype == goal.dtype == agent.dtype == torch.int32
        assert tuple(walls.shape) == (Cn, self.size) and tuple(goal.shape) == (Cn, 2) and tuple(agent.shape) == (Cn, 4)
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_replace_levels(self._h, nat.ptr(slots), nat.ptr(walls), nat.ptr(goal),
                                                          nat.ptr(agent), Cn, self._stream),
                      "merlin_env_replace_levels")

    def level_bank(self):
        """(walls int32[L, size], goal int32[L, 2], agent int32[L, 4]): the bound bank as the resets read it, copied out
        in snapshot()'s layouts (merlin_env_level_bank: one kernel, capturable)."""
        L = max(self.num_levels, 1)
        walls = torch.empty((L, self.size), dtype=torch.int32, device=self.device)
        goal = torch.empty((L, 2), dtype=torch.int32, device=self.device)
        agent = torch.empty((L, 4), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_level_bank(self._h, nat.ptr(walls), nat.ptr(goal), nat.ptr(agent),
                                                      self._stream), "merlin_env_level_bank")
        return walls, goal, agent

    def set_refill_interval(self, every: int) -> None:
        """Refill the used look-ahead map slots every `every` step calls (default 16); 0 leaves the
        refills to the caller's refill() (merlin_env_set_refill_interval)."""
        nat.check(self._lib.merlin_env_set_refill_interval(self._h, int(every)), "merlin_env_set_refill_interval")

    def set_step_fallback(self, on: bool) -> None:
        """on=False: the caller refills every used look-ahead slot after every step (refill(), refill interval 0),
        so the per-step fallback pass is not launched; a reset that meets an empty slot then raises
        DEVERR_SLOT_EMPTY in errors() (merlin_env_set_step_fallback)."""
        nat.check(self._lib.merlin_env_set_step_fallback(self._h, 1 if on else 0), "merlin_env_set_step_fallback")
        self.step_fallback = bool(on)

    def set_lookahead_depth(self, depth: int) -> None:
        """A ring of `depth` look-ahead maps per env (merlin_env_set_lookahead_depth; default 1, the single slot):
        refill() tops every ring up until it is full, a reset takes the oldest map, and a ring that is full when a
        caller starts serves `depth` resets per env with no refill in between.  At depth > 1 with refill interval 0
        reset() is not followed by a refill.  Results are the same at every depth.  Reallocates the ring
        (num_envs x depth x 104 B up to size 16, 168 B above), drops every look-ahead map and synchronises the
        device: not inside a graph capture, and a graph captured before it must be captured again."""
        self.join_refill()
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_set_lookahead_depth(self._h, int(depth)), "merlin_env_set_lookahead_depth")
        self.lookahead_depth = int(depth)

    def lookahead_bytes(self, depth: int) -> int:
        """Device bytes of a ring of `depth` look-ahead maps per env (rows, agent + goal, RNG state)."""
        return self.num_envs * int(depth) * (4 * (16 if self.size <= 16 else 32) + 40)

    def refill(self, stream=None) -> None:
        """Generate maps until every env's look-ahead ring is full again (at depth 1: the next map of every env
        whose slot was used), on the current stream (merlin_env_refill).  Touches only the rings and reads the
        envs' RNG: at depth 1 it may run on a side stream beside work that does not step this env, joined before
        the next step.  `stream`: run it on that stream behind the work queued on the current one; whatever next
        seeds, resets, steps or refills this env through this object waits for it first (join_refill; a captured
        graph that steps the env is the caller's to order: join_refill() before its replay)."""
        self.join_refill()
        if stream is None:
            with torch.cuda.device(self.device):
                nat.check(self._lib.merlin_env_refill(self._h, self._stream), "merlin_env_refill")
            return
        stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            nat.check(self._lib.merlin_env_refill(self._h, self._stream), "merlin_env_refill")
        self._topup = stream

    @property
    def refill_pending(self) -> bool:
        """A refill(stream=...) has been launched and nothing has waited for it yet."""
        return self._topup is not None

    def join_refill(self) -> None:
        """The current stream waits for a refill(stream=...) still pending; nothing to do otherwise."""
        if self._topup is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._topup)
            self._topup = None

    def step(self, actions: torch.Tensor, autoreset: bool = True):
        """gym-vector style step: returns (obs codes, reward, terminated, truncated, info).

        With autoreset the obs of a finished env is already the first obs of its next
        episode (src/ppo.py:93-98 resets on done before the next act)."""
        actions = actions.to(device=self.device, dtype=torch.int64).contiguous()
        self.step_into(actions, self.obs, self._rew, self._term, self._trunc, None, self._epr, self._epl,
                       autoreset=autoreset)
        info = {"episode_return": self._epr, "episode_length": self._epl}
        return self.obs, self._rew, self._term.bool(), self._trunc.bool(), info

    # -- observation rendering ------------------------------------------------
    def render_obs(self, codes: torch.Tensor | None = None, index: torch.Tensor | None = None,
                   out: torch.Tensor | None = None, scale: float = 1.0, layout: str = "nchw"):
        codes = self.obs if codes is None else codes
        return nat.expand_obs(codes.reshape(-1, nat.OBS_WORDS), index=index, out=out, scale=scale,
                              layout=layout)

    def render_rgb(self, codes: torch.Tensor | None = None) -> torch.Tensor:
        codes = self.obs if codes is None else codes
        return nat.expand_obs_u8(codes.reshape(-1, nat.OBS_WORDS))

    def flat_obs(self, codes: torch.Tensor | None = None, index: torch.Tensor | None = None) -> torch.Tensor:
        """f32 [n, D]: FlattenObservation of the wrapped observation as the reference's MLP path takes it (src/ppo.py:
        58-62: the uint8 values as floats, no scaling) -- the RGB partial view expanded from tile codes (rows `index`
        of `codes`, default the current ones), D = 9,408."""
        codes = self.obs if codes is None else codes
        return nat.expand_obs_u8(codes.reshape(-1, nat.OBS_WORDS), index=index).view(-1, 56 * 56 * 3).float()

    def render_full(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8[N, size, size, 3]: the fully observable observation of every env's current state
        (observation.fully_observable: FullyObsWrapper + ImgObsWrapper, src/scenario_creator/scenario_creator.py:45-50),
        out[i, x, y] = (object, color, state) of cell (x, y) as minigrid's Grid.encode, the agent's cell (10, 0, dir)
        (merlin_env_full_obs)."""
        S = self.size
        if out is None:
            out = torch.empty((self.num_envs, S, S, 3), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == self.num_envs * S * S * 3
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_full_obs(self._h, nat.ptr(out), self._stream), "merlin_env_full_obs")
        return out

    def render_frames(self, tile_size: int = 32, highlight: bool = True, index: torch.Tensor | None = None,
                      out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8[n, size*ts, size*ts, 3] on the device: minigrid's render() in rgb_array mode -- get_frame(highlight,
        tile_size), the whole grid at ts-pixel tiles, the agent's triangle in its world direction, the cells its view
        shows brightened -- of every env's current state, or of the envs `index` (int64 env ids) (merlin_env_render).
        `out`: a contiguous uint8 tensor of exactly that many bytes."""
        ts = int(tile_size)
        if index is not None:
            index = index.to(device=self.device, dtype=torch.int64).contiguous()
        n = self.num_envs if index is None else int(index.numel())
        side = self.size * max(ts, 0)
        if out is None:
            out = torch.empty((n, side, side, 3), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != n * side * side * 3:
            raise nat.MerlinNativeError(f"render_frames: out must be a contiguous uint8 tensor of "
                                        f"{n}x{side}x{side}x3 bytes")
        with torch.cuda.device(self.device), nat.KernelTimer.span("k_render_frames", out.numel() + n * 80):
            nat.check(self._lib.merlin_env_render(self._h, nat.ptr(index), n, ts, int(bool(highlight)), nat.ptr(out),
                                                  self._stream), "merlin_env_render")
        return out.view(n, side, side, 3)

    def snapshot(self):
        """(walls int32[N, size] bit rows, goal int32[N, 2], agent int32[N, 4] = x, y, dir, 0) of the current state
        as new device tensors, in the layouts merlin._native.render_frames takes (merlin_env_snapshot: one kernel, no
        host sync)."""
        n, S = self.num_envs, self.size
        walls = torch.empty((n, S), dtype=torch.int32, device=self.device)
        goal = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        agent = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_snapshot(self._h, nat.ptr(walls), nat.ptr(goal), nat.ptr(agent),
                                                    self._stream), "merlin_env_snapshot")
        return walls, goal, agent

    # -- shortest action paths (merlin/pathing.py) -----------------------------
    def optimal_steps(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """int32[N]: the least number of actions after which each env, from its current pose, can terminate at its
        goal; -1 if none does (merlin_env_optimal_steps: one kernel, no allocation beyond `out`, no host sync; reads
        the maps and poses only)."""
        return self._optimal(out, None)

    def distance_field(self, out: torch.Tensor | None = None):
        """(dist int32[N], field int16[N, 4, size, size]): optimal_steps() and the same distance for every pose of
        each env's map, indexed [dir][y][x]; -1 for walls and poses the goal cannot be reached from.  `out`: the
        field's buffer, a contiguous int16 tensor of that many elements at any alignment."""
        S = self.size
        if out is None:
            out = torch.empty((self.num_envs, 4, S, S), dtype=torch.int16, device=self.device)
        if out.dtype != torch.int16 or not out.is_contiguous() or out.numel() != self.num_envs * 4 * S * S:
            raise nat.MerlinNativeError(f"distance_field: out must be a contiguous int16 tensor of "
                                        f"{self.num_envs}x4x{S}x{S} elements")
        return self._optimal(None, out), out

    def _optimal(self, out, field):
        n = self.num_envs
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=self.device)
        if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() != n:
            raise nat.MerlinNativeError(f"optimal_steps: out must be a contiguous int32 tensor of {n} elements")
        with torch.cuda.device(self.device), nat.KernelTimer.span(
                "k_shortest_paths", nat.shortest_paths_bytes(n, self.size, field is not None)):
            nat.check(self._lib.merlin_env_optimal_steps(self._h, nat.ptr(out), nat.ptr(field), self._stream),
                      "merlin_env_optimal_steps")
        return out

    # -- introspection (host syncs; tests / tooling) --------------------------
    def get_state(self) -> dict:
        n, S = self.num_envs, self.size
        walls = np.zeros((n, S), dtype=np.uint32)
        agent = np.zeros((n, 8), dtype=np.int32)
        rng = np.zeros((n, 5), dtype=np.uint64)
        vp = C.c_void_p
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_get_state(self._h, walls.ctypes.data_as(vp), agent.ctypes.data_as(vp),
                                                     rng.ctypes.data_as(vp), self._stream), "merlin_env_get_state")
        cells = ((walls[:, :, None] >> np.arange(S, dtype=np.uint32)[None, None, :]) & 1).astype(np.uint8)
        cells[np.arange(n), agent[:, 5], agent[:, 4]] = np.where(
            cells[np.arange(n), agent[:, 5], agent[:, 4]] == 0, 2, cells[np.arange(n), agent[:, 5], agent[:, 4]])
        return {"walls": walls, "cells": cells, "agent_pos": agent[:, 0:2].copy(), "agent_dir": agent[:, 2].copy(),
                "step_count": agent[:, 3].copy(), "goal_pos": agent[:, 4:6].copy(), "stay": agent[:, 6].copy(),
                "rng": rng}

    def errors(self, raise_on_error: bool = True):
        flags, fb = C.c_uint32(), C.c_uint32()
        with torch.cuda.device(self.device):
            nat.check(self._lib.merlin_env_errors(self._h, C.byref(flags), C.byref(fb), self._stream),
                      "merlin_env_errors")
        if raise_on_error and flags.value:
            what = []
            if flags.value & nat.DEVERR_BAD_ACTION:
                what.append("action outside {0,1,2} (ThreeActionWrapper IndexError; -1 = the policy's "
                            "logits were non-finite, merlin_act_heads)")
            if flags.value & nat.DEVERR_PLACE_OBJ:
                what.append("place_obj rejection sampling failed (RecursionError)")
            if flags.value & nat.DEVERR_SLOT_EMPTY:
                what.append("a reset met an empty look-ahead map slot with the step fallback off (refill() was not "
                            "run after every step)")
            if flags.value & nat.DEVERR_BAD_FRAME:
                what.append("render_frames was given an env id outside [0, num_envs) or met an agent off the grid")
            raise nat.MerlinNativeError("device env error: " + "; ".join(what))
        return flags.value, fb.value


class MerlinEnv:
    """Single MERLIN env with the gymnasium API the reference's PPO uses:
    ``reset(seed=None) -> (uint8[56,56,3], {})`` and
    ``step(a) -> (obs, float reward, bool terminated, bool truncated, {})``.

    Backed by a 1-env ``MerlinVecEnv`` (no auto-reset: the caller resets on done,
    as src/ppo.py:93-98 does).  Every step crosses the host boundary, like the
    reference on a GPU device (src/ppo.py:59,76); use ``MerlinVecEnv`` for speed.
    """

    def __init__(self, difficulty: str = "mediumhard", size: int = 16, device="cuda", fully_observable: bool = False,
                 flatten: bool = False, render_mode: str | None = None, **kw):
        if render_mode == "human":
            raise ValueError("render_mode='human' opens a window, which this library does not; use "
                             "render_mode='rgb_array' and render(), or ppo_visualization.py, which writes GIFs")
        if render_mode not in (None, "rgb_array"):
            raise ValueError(f"Unknown render_mode: {render_mode}")
        self.render_mode = render_mode
        self.vec = MerlinVecEnv(1, difficulty=difficulty, size=size, device=device, **kw)
        self.action_space = self.vec.action_space
        # the reference's observation options (src/config/scenario.yaml observation.*,
        # src/scenario_creator/scenario_creator.py:45-53): the RGB partial view (default) or the encoded full grid,
        # either flattened to a vector by FlattenObservation
        self.fully_observable, self.flatten = bool(fully_observable), bool(flatten)
        shape = (self.vec.size, self.vec.size, 3) if self.fully_observable else (56, 56, 3)
        if self.flatten:
            shape = (int(np.prod(shape)),)
        self.observation_space = Box(0, 255, shape, np.uint8)
        self.max_steps = self.vec.max_steps
        self._done = True

    @property
    def unwrapped(self):
        return self

    @property
    def agent_pos(self):
        return tuple(int(v) for v in self.vec.get_state()["agent_pos"][0])

    def _frame(self) -> np.ndarray:
        img = self.vec.render_full() if self.fully_observable else self.vec.render_rgb()
        img = img[0].cpu().numpy()
        return img.reshape(-1) if self.flatten else img

    def reset(self, seed: int | None = None, options=None):
        if seed is not None:
            self.vec.seed(int(seed) - self.vec.env_offset)
        self.vec.reset()
        self._done = False
        return self._frame(), {}

    def step(self, action):
        a = torch.tensor([int(action)], dtype=torch.int64, device=self.vec.device)
        _, rew, term, trunc, _ = self.vec.step(a, autoreset=False)
        flags, _ = self.vec.errors(raise_on_error=False)
        if flags & nat.DEVERR_BAD_ACTION:
            raise IndexError(f"action {action} is not in ThreeActionWrapper's {{0, 1, 2}}")
        r = float(rew[0].item())
        return self._frame(), r, bool(term[0].item()), bool(trunc[0].item()), {}

    def optimal_steps(self) -> int:
        """The least number of actions after which the env, from its current pose, can terminate at the goal; -1 if
        it cannot (MerlinVecEnv.optimal_steps)."""
        return int(self.vec.optimal_steps()[0].item())

    def get_frame(self, highlight: bool = True, tile_size: int = 32) -> np.ndarray:
        """minigrid's get_frame: the uint8[size*ts, size*ts, 3] picture of the whole grid in the current state."""
        return self.vec.render_frames(tile_size=tile_size, highlight=highlight)[0].cpu().numpy()

    def render(self) -> np.ndarray:
        """minigrid's render() in rgb_array mode: get_frame(highlight=True, tile_size=32)."""
        return self.get_frame()

    def close(self):
        self.vec.close()
