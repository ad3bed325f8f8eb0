"""Few-shot evaluation (src/distribution_over_tasks.py:132-209 evaluate_few_shot), batched over tasks.

Reference semantics kept, per unseen task (= one map seed):
  * the fast policy starts as a copy of the meta policy (:133-134);
  * ``adapt_steps`` times (:139-203): a support rollout of ``k_support`` sampled steps from
    ``reset(seed=task_seed)``, reset to the same seed at every done; FOMAML's loss on it (PPO clipped surrogate +
    0.5 value MSE - 0.05 entropy, GAE(.995, .95), advantages normalised over the rollout, returns = values +
    normalised advantages); clip_grad_norm_(0.5); one SGD(lr_inner) step;
  * then one deterministic episode from ``reset(seed=task_seed)`` with the adapted weights and its loss
    (:71-130): the episode's reward, its length, -mean(logp) + 0.5 mean((v - ret)^2).
MI355X batching: G tasks at once on a ``FOMAML`` instance whose meta policy is the given policy -- its
``collect_trajectory`` (grouped acting fused with the env step, one HIP graph per rollout shape), ``compute_loss``
(HIP GAE, grouped evaluate, every task's gradient from one autograd pass) are used as they are.  New here are the
two reductions behind the C ABI (csrc/merlin_fewshot.hip): the per-task clip + SGD (``nat.group_clip_sgd``, 2
launches for all tasks and tensors) and the per-episode GAE / normalisation / loss (``nat.episode_loss``, 1 launch).

Sampling: the support rollouts draw with the counter-keyed generator of merlin_env_act_step, keyed by (a 62-bit seed
taken from torch's generator when the adapter is constructed, the rollout counter, the step, the task's env index).
So the same ``torch.manual_seed`` and the same sequence of calls give identical results; and a task's draws depend on
its position among the tasks passed in one call (its env index), not on its seed alone.
"""
from __future__ import annotations

import torch

from . import _native as nat
from . import batched_policy as bp
from . import grouped_policy as gp
from .actor_critic import CNNActorCritic
from .fomaml import FOMAML

MAX_GRAD_NORM = 0.5  # src/distribution_over_tasks.py:202
EVAL_ROWS = 256  # the episodes are re-evaluated this many steps at a time (bounds the im2col buffers)
DONE_CHECK_EVERY = 64  # steps between the host's looks at the done flags


class FewShotAdapter:
    """Adapts a CNNActorCritic to batches of tasks and scores the adapted weights.  Per-task weights travel as
    stacks {parameter name: [G, *shape]} (merlin.batched_policy.stack_params)."""

    def __init__(self, ac, lr_inner: float = 0.01, difficulty: str = "mediumhard", size: int = 16, device="cuda",
                 max_steps: int | None = None, gamma: float = 0.995, lam: float = 0.95, **env_flags):
        if not isinstance(ac, CNNActorCritic):
            raise ValueError("few-shot evaluation supports CNNActorCritic policies on the RGB partial view only, "
                             f"got {type(ac).__name__}")
        env_kwargs = {"difficulty": difficulty, "size": int(size), "max_steps": max_steps, **env_flags}
        self.fm = FOMAML(None, lr_inner=lr_inner, device=device, difficulty=difficulty, meta_policy=ac,
                         env_kwargs=env_kwargs)
        self.fm.gamma, self.fm.lam = gamma, lam
        self.ac = ac
        self.lr_inner = lr_inner
        self.device = self.fm.device
        self.names = [n for n, _ in ac.named_parameters()]
        self._graph_env = {}  # rollout key -> the env its HIP graph was recorded on

    def close(self):
        if self.fm._env is not None:
            self.fm._rollouts.clear()
            self.fm._kept.clear()
            self.fm._env.close()
            self.fm._env = None

    def meta_params(self, G: int) -> dict:
        """Every task's copy of the meta policy."""
        return {n: p.detach() for n, p in bp.stack_params(self.ac, G).items()}

    def adapt_step(self, batch, params=None, lr_inner: float | None = None) -> dict:
        """One inner step on a support batch ([k][G], as FOMAML.collect_trajectory returns it): compute_loss, every
        task's gradient from one autograd pass, per-task clip_grad_norm_(0.5) + SGD (merlin_group_clip_sgd).
        params None: every task starts from the meta policy.  Returns new detached stacks; params is not changed."""
        G = int(batch["rew"].shape[1])
        lr = self.lr_inner if lr_inner is None else lr_inner
        if params is None:
            fast = bp.stack_params(self.ac, G)
        else:
            fast = {n: params[n].detach().clone().requires_grad_(True) for n in self.names}
        loss, _ = self.fm.compute_loss(batch, fast)
        grads = torch.autograd.grad(loss, [fast[n] for n in self.names])
        new = [fast[n].detach() for n in self.names]
        nat.group_clip_sgd(new, [g.contiguous() for g in grads], lr, MAX_GRAD_NORM)
        return dict(zip(self.names, new))

    def adapt(self, task_seeds, adapt_steps: int, k_support: int, task_difficulties=None) -> dict:
        """adapt_steps x (support rollout of k_support sampled steps of every task with its current weights, then
        adapt_step).  adapt_steps = 0: the meta stacks.  task_difficulties: one difficulty name per task (None: the
        adapter's difficulty for all); the rollout graphs read the classes from the env's class buffer, so changing
        them between calls needs no re-capture (FOMAML._task_env)."""
        G = len(task_seeds)
        params = self.meta_params(G)
        if adapt_steps <= 0:
            return params
        env = self.fm._task_env(task_seeds, task_difficulties)
        # the rollout state is looked up by the key alone: the key carries the shape, and a graph recorded on an env
        # that has since been replaced (another G in between) is dropped
        key = f"fs{G}x{int(k_support)}"
        if self._graph_env.get(key) is not env:
            self.fm._rollouts.pop(key, None)
            self._graph_env[key] = env
        for _ in range(adapt_steps):
            batch = self.fm.collect_trajectory(env, params, int(k_support), key=key, host_stats=False)
            params = self.adapt_step(batch, params)
        env.errors()
        return params

    @torch.no_grad()
    def episode(self, params, task_seeds, max_steps: int | None = None, record: bool = False,
                task_difficulties=None):
        """One deterministic episode per task with its own weights -> (rewards list[float], steps list[int], losses
        list[float]) [+ actions int64 [T, G] on the host when record].  A task's result is frozen at its first done
        (the env then replays the same map; those steps are ignored); a task still running after max_steps (default
        and at most the env's) counts its steps and rewards so far.  task_difficulties: as adapt."""
        G = len(task_seeds)
        env = self.fm._task_env(task_seeds, task_difficulties)
        cap = env.max_steps if not max_steps else min(int(max_steps), env.max_steps)
        dev = self.device
        pk = gp.pack(params)
        A = int(pk["ba_r"].shape[1])
        codes = torch.zeros((cap + 1, G, 8), dtype=torch.int32, device=dev)
        act = torch.zeros((cap, G), dtype=torch.int64, device=dev)
        logp = torch.zeros((cap, G), dtype=torch.float32, device=dev)
        val = torch.zeros((cap, G), dtype=torch.float32, device=dev)
        rew = torch.zeros((cap, G), dtype=torch.float32, device=dev)
        done = torch.zeros((cap, G), dtype=torch.float32, device=dev)
        epr = torch.zeros((cap, G), dtype=torch.float64, device=dev)
        epl = torch.zeros((cap, G), dtype=torch.int32, device=dev)
        part = torch.zeros((2, 8, G, 4), dtype=torch.float32, device=dev)
        a3ws = torch.zeros((2 * G, 576), dtype=torch.float32, device=dev)
        zb = torch.zeros(4, dtype=torch.float32, device=dev)
        env.reset(out=codes[0])
        T = 0
        while T < cap:
            gp.act_parts(pk, codes[T], part=part, a3_ws=a3ws)
            env.act_step_into(part, zb[:A], zb[:1], (act[T], logp[T], val[T]), codes[T + 1], rew[T], None, None,
                              done[T], epr[T], epl[T], deterministic=True)
            T += 1
            if (T % DONE_CHECK_EVERY == 0 or T == cap) and bool((done[:T].sum(0) > 0).all()):
                break
        env.errors()
        d = done[:T] > 0
        ended = d.any(0)
        first = d.int().argmax(0)  # the first done's step
        steps = torch.where(ended, first + 1, torch.full_like(first, T))
        total = torch.where(ended, epr[:T].gather(0, first.unsqueeze(0)).squeeze(0), rew[:T].double().sum(0))
        Tm = int(steps.max().item())
        new_logp = torch.empty((Tm, G), dtype=torch.float32, device=dev)
        new_val = torch.empty((Tm, G), dtype=torch.float32, device=dev)
        for t0 in range(0, Tm, EVAL_ROWS):  # every task's rows t0 .. t1 - 1, padded to the longest episode
            t1 = min(t0 + EVAL_ROWS, Tm)
            rows = codes[t0:t1].transpose(0, 1).reshape(G * (t1 - t0), 8).contiguous()  # task-major
            lp, _, nv = gp.evaluate(params, rows, t1 - t0, act[t0:t1].t())
            new_logp[t0:t1] = lp.t()
            new_val[t0:t1] = nv.t()
        loss = nat.episode_loss(rew[:Tm], val[:Tm], new_logp, new_val, steps.to(torch.int32).contiguous(),
                                self.fm.gamma, self.fm.lam)
        out = (total.cpu().tolist(), steps.cpu().tolist(), loss.cpu().tolist())
        if record:
            out = out + (act[:T].cpu(),)
        return out
