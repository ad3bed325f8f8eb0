"""Probe: the per-update planning of PPO._sgd at the bench state (merlin.dedup.FrameGroups, merlin.windows.WindowPlan,
WindowPlan.update_minibatches(bulk=True)).  Per stage: wall time with the stream drained around it (median of `reps`),
and from one more pass under torch.profiler the GPU-busy time (sum of the kernel and memcpy durations: the stages run
on one stream, so nothing overlaps) and the launch count.  The bulk stage is also touched the way the update touches
it (every minibatch's attributes read once), so a builder that defers its views pays for them here too.
    python scripts/probe_plan.py [warm iterations] [reps] [native: 0 | 1]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-2dgrid_amd"))
import torch

from merlin import MerlinVecEnv
from merlin import windows as W
from merlin.dedup import FrameGroups
from merlin.ppo import PPO
from merlin.windows import WindowPlan


def touch(mbs):
    for ep in mbs:
        for mb in ep:
            for a in ("groups", "inv", "slot", "order", "offs", "kmap", "rep_row"):
                getattr(mb, a)


def gpu_busy(fn):
    """(GPU-busy ms, launches) of fn() from the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    us, n = 0.0, 0
    for ev in prof.events():
        if str(ev.device_type).endswith("CUDA"):
            us += ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
            n += 1
    return round(us / 1e3, 3), n


def main():
    warm = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if len(sys.argv) > 3 and hasattr(W, "NATIVE_PLAN"):
        W.NATIVE_PLAN = bool(int(sys.argv[3]))
    native = getattr(W, "NATIVE_PLAN", False)
    dev = torch.device("cuda", 0)
    env = MerlinVecEnv(4096, "mediumhard", seed=777, device=dev)
    torch.manual_seed(777)
    agent = PPO(env, batch_size=4096 * 256, minibatch_size=4096 * 256 // 8, ent_coef=0.05, device=dev)
    for _ in range(warm):
        agent.update(agent.collect_rollouts())
    agent.collect_rollouts()
    codes = agent.buf.flat_codes
    B = codes.shape[0]
    perms = [torch.randperm(B, device=dev) for _ in range(10)]
    ts = {"FrameGroups": [], "WindowPlan": [], "update_minibatches": [], "update_minibatches+views": [],
          "update_minibatches(lazy)": []}
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if native:  # one call builds both; reported under WindowPlan
            fg, plan = WindowPlan.native(codes)
            t1 = t0
        else:
            fg = FrameGroups(codes)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            plan = WindowPlan(codes, fg)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        mbs = plan.update_minibatches(perms, B // 8, bulk=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        touch(mbs)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        plan.update_minibatches(perms, B // 8, bulk=False)
        torch.cuda.synchronize()
        ts["update_minibatches(lazy)"].append((time.perf_counter() - t4) * 1e3)
        ts["FrameGroups"].append((t1 - t0) * 1e3)
        ts["WindowPlan"].append((t2 - t1) * 1e3)
        ts["update_minibatches"].append((t3 - t2) * 1e3)
        ts["update_minibatches+views"].append((t4 - t2) * 1e3)
    print("native plan:", getattr(W, "NATIVE_PLAN", None))
    print("wall ms, stream drained:", {k: round(statistics.median(v), 2) for k, v in ts.items()},
          f"frames {plan.num_frames} windows {plan.num_windows} patches {plan.num_patches} bands {plan.num_bands}",
          flush=True)
    try:
        busy = {"FrameGroups": (0.0, 0) if native else gpu_busy(lambda: FrameGroups(codes)),
                "WindowPlan": gpu_busy((lambda: WindowPlan.native(codes)) if native else
                                       (lambda: WindowPlan(codes, fg))),
                "update_minibatches+views": gpu_busy(lambda: touch(plan.update_minibatches(perms, B // 8, bulk=True)))}
        print("(GPU-busy ms, launches):", busy, flush=True)
    except Exception as e:  # the profiler is optional: the wall times above stand without it
        print("profiler unavailable:", repr(e), flush=True)


if __name__ == "__main__":
    main()
