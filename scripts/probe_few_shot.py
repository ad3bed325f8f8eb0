"""Few-shot evaluation's two reductions against the torch chains they replace, and evaluate_few_shot's wall time.

  clip+sgd   nat.group_clip_sgd (2 launches) vs FOMAML._clip_per_task + fast - lr * g (~80 launches), G = 32 on the
             model's 20 parameter tensors, alternated in one process, median of 20 after warm-up
  ep. loss   nat.episode_loss (1 launch) vs the GAE / normalisation / index_add_ reduction of
             merlin/evaluation.py evaluate_zero_shot (given the re-evaluated logp / value), n = 512, T = 1024
  wall       evaluate_few_shot at the reference CLI's defaults (500 tasks, k_support 256), adapt_steps 1 and 3,
             after a one-chunk warm-up (code objects, GEMM algorithm choice)

python scripts/probe_few_shot.py [tasks]      (tasks 0: kernels only)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-2dgrid_amd"))
import torch

from merlin import _native as nat
from merlin import batched_policy as bp
from merlin.actor_critic import CNNActorCritic
from merlin.evaluation import evaluate_few_shot
from merlin.fomaml import FOMAML

REPS = 20


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab(name, fa, fb, na="hip", nb="torch"):
    for _ in range(3):
        fa(), fb()
    ta, tb = [], []
    for _ in range(REPS):  # alternated: both see the same neighbours on the machine
        ta.append(timed_ms(fa))
        tb.append(timed_ms(fb))
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(f"{name}: {na} median {ma * 1e3:.1f} us (min {min(ta) * 1e3:.1f}, max {max(ta) * 1e3:.1f})  "
          f"{nb} median {mb * 1e3:.1f} us (min {min(tb) * 1e3:.1f}, max {max(tb) * 1e3:.1f})  ratio {mb / ma:.2f}x",
          flush=True)


def probe_clip_sgd(dev, ac, G=32, lr=0.01):
    fast = {n: p.detach() for n, p in bp.stack_params(ac, G).items()}
    names = list(fast)
    grads = {n: torch.randn_like(fast[n]) * 0.01 for n in names}
    ps = [fast[n].clone() for n in names]
    gs = [grads[n].clone() for n in names]
    norm = torch.empty(G, device=dev)
    numel = sum(p[0].numel() for p in ps)
    ws = torch.empty(int(nat.lib().merlin_group_clip_sgd_workspace(
        len(ps), (nat.C.c_int64 * len(ps))(*[p[0].numel() for p in ps]), G)), dtype=torch.float64, device=dev)

    def hip():
        nat.group_clip_sgd(ps, gs, lr, 0.5, norm_out=norm, workspace=ws)

    def chain():
        clipped, _ = FOMAML._clip_per_task(grads, 0.5)
        return {n: fast[n] - lr * clipped[n] for n in names}

    print(f"clip+sgd: G {G}, {len(ps)} tensors, {numel} parameters per task, "
          f"{G * numel * 20 / 1e6:.1f} MB moved by the two launches")
    ab("clip+sgd", hip, chain)


def probe_episode_loss(dev, n=512, T=1024, gamma=0.995, lam=0.95):
    g = torch.Generator(device=dev).manual_seed(1)
    rew, V, nlp, nv = (torch.randn(T, n, device=dev, generator=g) for _ in range(4))
    steps = torch.randint(1, T + 1, (n,), device=dev, generator=g)
    length = steps.to(torch.int32)
    ws = torch.empty(T, n, device=dev)
    out = torch.empty(n, device=dev)

    def hip():
        nat.episode_loss(rew, V, nlp, nv, length, gamma, lam, workspace=ws, out=out)

    def chain():  # evaluate_zero_shot's reduction, with the re-evaluated logp / value given
        t_idx = torch.arange(T, device=dev).unsqueeze(1)
        valid = t_idx < steps.unsqueeze(0)
        last = (t_idx == (steps - 1).unsqueeze(0)).float()
        adv, _ = nat.gae(rew, V, last.contiguous(), torch.zeros(n, device=dev), gamma, lam)
        cnt = steps.clamp_min(1).to(torch.float32)
        zero = torch.zeros((), device=dev)
        mean = torch.where(valid, adv, zero).sum(0) / cnt
        var = torch.where(valid, (adv - mean) ** 2, zero).sum(0) / (cnt - 1).clamp_min(1)
        adv_n = torch.where((steps > 1).unsqueeze(0), (adv - mean) / (var.sqrt() + 1e-8), zero)
        ret = V + adv_n
        sel = valid.reshape(-1)
        env_of = torch.arange(n, device=dev).repeat(T)[sel]
        lp_mean = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, env_of, nlp.reshape(-1)[sel].double())
        v_err = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(
            0, env_of, ((nv.reshape(-1)[sel] - ret.reshape(-1)[sel]) ** 2).double())
        return (-lp_mean / cnt + 0.5 * v_err / cnt).float()

    hip()
    d = (out - chain()).abs().max().item()
    print(f"episode loss: n {n}, T {T}, mean length {steps.float().mean().item():.0f}, max |hip - torch| {d:.2e}")
    ab("episode loss", hip, chain)


def probe_wall(dev, ac, tasks):
    seeds = list(range(100000, 100000 + tasks))
    evaluate_few_shot(ac, seeds[:32], 1, device=dev)  # warm-up: one chunk
    for steps in (1, 3):
        torch.manual_seed(0)
        ms = timed_ms(lambda: evaluate_few_shot(ac, seeds, steps, device=dev))
        print(f"evaluate_few_shot: {tasks} tasks, k_support 256, adapt_steps {steps}: {ms / 1e3:.2f} s "
              f"({ms / tasks:.1f} ms per task)", flush=True)


def main():
    tasks = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ac = CNNActorCritic((56, 56, 3), 3).to(dev)
    probe_clip_sgd(dev, ac)
    probe_episode_loss(dev)
    if tasks > 0:
        probe_wall(dev, ac, tasks)


if __name__ == "__main__":
    main()
