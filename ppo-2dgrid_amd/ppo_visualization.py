"""Episode playback CLI -- the reference's ppo/ppo_visualization.py (flags :15-24), writing files instead of opening
a PyGame window, and with --adapt_steps the before / after playback of its fomaml/fomaml_visualization.py.

    python ppo-2dgrid_amd/ppo_visualization.py --difficulty hard --episodes 10 --out_dir renders/

The newest best_model.pth under --ckpt_dir whose path names the difficulty's env id is loaded (or --model_path),
episode ep = 1..episodes is played deterministically on the map of seed `seed + ep` (`ep` when seed is 0), and the
per-episode and average lines of the reference are printed.  All episodes run in ONE batched pass on the GPU envs
(merlin.recording.record_episodes); each is then written as <out_dir>/episode_<ep>_seed_<s>.gif (or the compact
.npz recording with --format npz) together with summary.png, a contact sheet of every episode's final state.
--no-render only prints.

--adapt_steps K: every seed is played before and after K few-shot adaptation steps on its own map
(merlin.few_shot.FewShotAdapter: clipped SGD(--lr_inner) on --k_support sampled steps each); both recordings are
written (episode_<ep>_seed_<s>_pre.gif / _post.gif, summary_pre.png / summary_post.png).
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from merlin.checkpoints import load_policy  # noqa: E402
from merlin.recording import Recording, record_episodes  # noqa: E402
from merlin.scenario_creator import DEFAULT_CONFIG, ScenarioCreator  # noqa: E402
from merlin.utils.utils import get_device  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--difficulty", type=str, default="easy",
                   choices=["easy", "medium", "mediumhard", "hard", "hardest"])
    p.add_argument("--episodes", type=int, default=10)
    p.add_argument("--model_path", type=str, default=None)
    p.add_argument("--ckpt_dir", type=str, default="checkpoints")
    p.add_argument("--config", type=str, default=DEFAULT_CONFIG)
    p.add_argument("--no-render", action="store_true", help="only print the results, write no files")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--out_dir", type=str, default="renders/")
    p.add_argument("--tile_size", type=int, default=32, help="pixels per grid cell, 4..32")
    p.add_argument("--fps", type=int, default=20)
    p.add_argument("--format", type=str, default="gif", choices=["gif", "npz"])
    p.add_argument("--max_steps", type=int, default=None, help="episode step limit (default 4 * size^2)")
    p.add_argument("--adapt_steps", type=int, default=0, help="K > 0: also play every seed after K adaptation steps")
    p.add_argument("--lr_inner", type=float, default=0.01)
    p.add_argument("--k_support", type=int, default=256)
    return p.parse_args(argv)


def find_latest_checkpoint(ckpt_root: str, name_filter: str) -> str:
    """The most recently written best_model.pth below ckpt_root whose path contains name_filter."""
    if not os.path.exists(ckpt_root):
        raise FileNotFoundError(f"Missing directory: {ckpt_root}")
    found = [m for m in glob.glob(os.path.join(ckpt_root, "**", "best_model.pth"), recursive=True)
             if not name_filter or name_filter in m]
    if not found:
        raise FileNotFoundError(f"No models found matching filter: {name_filter}")
    return max(found, key=os.path.getmtime)


def report(rec: Recording, title: str = "") -> None:
    if title:
        print(title)
    rewards, steps = rec.returns.tolist(), rec.lengths.tolist()
    for ep, (r, s) in enumerate(zip(rewards, steps), 1):
        print(f"Episode {ep:>2} | Reward: {r:.3f} | Steps: {s}")
    print("-" * 40)
    print(f"Average Reward: {np.mean(rewards):.3f}")
    print(f"Average Steps : {np.mean(steps):.1f}")
    print("-" * 40)


def write_files(rec: Recording, args, suffix: str = "") -> list:
    os.makedirs(args.out_dir, exist_ok=True)
    written = []
    for i, s in enumerate(rec.seeds):
        stem = os.path.join(args.out_dir, f"episode_{i + 1}_seed_{s}{suffix}")
        if args.format == "gif":
            written.append(rec.save_gif(stem + ".gif", i, fps=args.fps, tile_size=args.tile_size))
        else:
            one = Recording(rec.seeds[i:i + 1], rec.difficulty if isinstance(rec.difficulty, str) else
                            rec.difficulty[i:i + 1], rec.size, rec.max_steps, rec.walls[i:i + 1], rec.goal[i:i + 1],
                            rec.agent[:, i:i + 1], rec.actions[:, i:i + 1], rec.rewards[:, i:i + 1],
                            rec.lengths[i:i + 1], rec.returns[i:i + 1], device=rec.device)
            written.append(one.save_npz(stem + ".npz"))
    sheet = rec.contact_sheet(tile_size=min(args.tile_size, 16))
    path = os.path.join(args.out_dir, f"summary{suffix}.png")
    try:
        from PIL import Image

        Image.fromarray(sheet).save(path)
    except ImportError:
        path = path[:-4] + ".npy"
        np.save(path, sheet)
        print(f"PIL is not installed: wrote the contact sheet as {path}")
    written.append(path)
    return written


def adapted_recordings(policy, seeds, args, size, device):
    """(before, after): every seed played with the loaded policy, and with its own copy after --adapt_steps steps."""
    from merlin.few_shot import FewShotAdapter

    ad = FewShotAdapter(policy, lr_inner=args.lr_inner, difficulty=args.difficulty, size=size, device=device,
                        max_steps=args.max_steps)
    try:
        out = []
        for k in (0, args.adapt_steps):
            params = ad.adapt(seeds, k, args.k_support)
            rew, steps, _, actions = ad.episode(params, seeds, record=True)
            rec = Recording.from_actions(seeds, actions, difficulty=args.difficulty, size=size,
                                         max_steps=args.max_steps, device=device)
            if rec.lengths.tolist() != list(steps) or rec.returns.tolist() != list(rew):
                raise RuntimeError("the replay of the recorded actions did not reproduce the adapted episode")
            out.append(rec)
        return out
    finally:
        ad.close()


def main(argv=None):
    args = parse_args(argv)
    device = get_device("auto")
    sc = ScenarioCreator(args.config)
    size = int(sc.get_env_size_str(args.difficulty).split("x")[0])
    model_path = args.model_path or find_latest_checkpoint(args.ckpt_dir, sc.get_env_id(args.difficulty))
    print(f"\n[*] Loading model: {model_path}")
    policy = load_policy(model_path, device)
    print(f"[*] Starting Evaluation ({args.episodes} Episodes)...\n")
    seeds = [args.seed + ep if args.seed else ep for ep in range(1, args.episodes + 1)]
    written = []
    if args.adapt_steps > 0:
        pre, post = adapted_recordings(policy, seeds, args, size, device)
        report(pre, "[*] Before adaptation")
        report(post, f"[*] After {args.adapt_steps} adaptation step(s)")
        if not args.no_render:
            written = write_files(pre, args, "_pre") + write_files(post, args, "_post")
    else:
        rec = record_episodes(policy, seeds, difficulty=args.difficulty, size=size, device=device,
                              max_steps=args.max_steps)
        report(rec)
        if not args.no_render:
            written = write_files(rec, args)
    if written:
        print(f"[*] Wrote {len(written)} files to {args.out_dir}")
    return written


if __name__ == "__main__":
    main()
