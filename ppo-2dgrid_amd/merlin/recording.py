"""Recorded episodes and their pictures.

``Recording``        the trajectory of one deterministic episode per seed, compact: each env's map once (there is no
                     auto-reset in evaluation), the agent's (x, y, dir) at every step, the actions, the per-step
                     rewards, the episode lengths and returns.  Pixels are made on demand by the full-grid renderer
                     (merlin_render_frames: minigrid's render() in rgb_array mode), a chunk of frames per launch.
``Recording.from_actions``  replays recorded actions int64[T, n] -- what ``evaluate_seeds(record=True)`` and
                     ``FewShotAdapter.episode(record=True)`` return -- through a ``MerlinVecEnv(seeds=...)`` without
                     auto-reset, one ``snapshot()`` per step; an env's trajectory is frozen at its first done.
``record_episodes``  evaluate, then replay.

The reference shows episodes in a PyGame window (ppo/ppo_visualization.py, fomaml/fomaml_visualization.py:
``render_mode="human"``); here they become GIF files, or the compact ``.npz`` a later session renders.
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import _native as nat
from .envs import MerlinVecEnv
from .evaluation import _per_seed, evaluate_seeds


class Recording:
    # frames rendered per launch are capped at this many bytes (a 1,024-step episode of a 16x16 grid at 32 px is
    # 805 MB of pixels): frames() and save_gif() stream chunk by chunk
    chunk_bytes = 256 << 20

    def __init__(self, seeds, difficulty, size, max_steps, walls, goal, agent, actions, rewards, lengths, returns,
                 device="cuda"):
        self.seeds = [int(s) for s in seeds]
        self.difficulty = difficulty if isinstance(difficulty, str) else [str(d) for d in difficulty]
        self.size, self.max_steps = int(size), int(max_steps)
        self.walls = torch.as_tensor(walls, dtype=torch.int32).cpu().contiguous()      # [n, size] bit rows
        self.goal = torch.as_tensor(goal, dtype=torch.int32).cpu().contiguous()        # [n, 2]
        self.agent = torch.as_tensor(agent, dtype=torch.int32).cpu().contiguous()      # [T + 1, n, 4] x, y, dir, 0
        self.actions = torch.as_tensor(actions, dtype=torch.int64).cpu().contiguous()  # [T, n]
        self.rewards = torch.as_tensor(rewards, dtype=torch.float32).cpu().contiguous()  # [T, n], 0 after the end
        self.lengths = torch.as_tensor(lengths, dtype=torch.int64).cpu().contiguous()  # [n] steps of the episode
        self.returns = torch.as_tensor(returns, dtype=torch.float64).cpu().contiguous()  # [n]
        self.device = torch.device(device)
        n = len(self.seeds)
        T = int(self.actions.shape[0])
        assert self.walls.shape == (n, self.size) and self.goal.shape == (n, 2) and self.agent.shape == (T + 1, n, 4)
        assert self.actions.shape == (T, n) == self.rewards.shape and self.lengths.shape == (n,) == self.returns.shape

    @property
    def num_envs(self) -> int:
        return len(self.seeds)

    # -- building ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_actions(cls, seeds, actions, difficulty="mediumhard", size: int = 16, max_steps: int | None = None,
                     device="cuda", **env_flags) -> "Recording":
        seeds = [int(s) for s in seeds]
        n = len(seeds)
        actions = torch.as_tensor(actions, dtype=torch.int64)
        assert actions.dim() == 2 and actions.shape[1] == n, "actions: int64[T, n]"
        env = MerlinVecEnv(n, difficulty=_per_seed(difficulty, n), size=size, device=device, max_steps=max_steps,
                           seeds=seeds, **env_flags)
        try:
            dev = env.device
            acts = actions.to(dev)
            env.reset()
            walls, goal, agent = env.snapshot()
            states, rews = [agent], []
            total = torch.zeros(n, dtype=torch.float64, device=dev)
            steps = torch.zeros(n, dtype=torch.int64, device=dev)
            done = torch.zeros(n, dtype=torch.bool, device=dev)
            for t in range(int(acts.shape[0])):
                _, rew, term, trunc, info = env.step(acts[t].contiguous(), autoreset=False)
                _, _, agent = env.snapshot()
                live = ~done
                states.append(torch.where(live[:, None], agent, states[-1]))  # frozen at the first done
                rews.append(torch.where(live, rew, torch.zeros((), device=dev)))
                total = torch.where(live & (term | trunc), info["episode_return"], total)
                steps += live.long()
                done |= term | trunc
                if bool(done.all()):
                    break
            env.errors()
            T = len(rews)
            rewards = torch.stack(rews) if T else torch.zeros((0, n))
            return cls(seeds, difficulty, size, env.max_steps, walls, goal, torch.stack(states), acts[:T], rewards,
                       steps, total, device=dev)
        finally:
            env.close()

    # -- shortest paths ---------------------------------------------------------------------------------------------
    def optimal_steps(self) -> torch.Tensor:
        """int64[n] on the host: the least number of actions after which each recorded episode could have terminated
        at its goal from its start pose, -1 where none does (merlin._native.shortest_paths on the recording's own maps;
        merlin/pathing.py has the metrics built on it)."""
        if not self.num_envs:
            return torch.zeros(0, dtype=torch.int64)
        dist = nat.shortest_paths(self.walls.to(self.device), self.goal.to(self.device),
                                  self.agent[0].contiguous().to(self.device), self.size)
        return dist.cpu().long()

    # -- pixels -----------------------------------------------------------------------------------------------------
    def _range(self, i: int, start: int, stop):
        last = int(self.lengths[i]) + 1  # step 0 is the reset state
        stop = last if stop is None else min(int(stop), last)
        return max(0, int(start)), max(max(0, int(start)), stop)

    def iter_frames(self, i: int, tile_size: int = 32, highlight: bool = True, start: int = 0, stop=None):
        """Env i's frames of steps [start, stop) (default: the whole episode, lengths[i] + 1 frames) as device
        tensors uint8[k, size*ts, size*ts, 3], one merlin_render_frames launch per chunk of at most chunk_bytes."""
        start, stop = self._range(i, start, stop)
        side = self.size * int(tile_size)
        per = max(1, int(self.chunk_bytes) // max(1, side * side * 3))
        walls = self.walls[i:i + 1].to(self.device)
        goal = self.goal[i:i + 1].to(self.device)
        for a in range(start, stop, per):
            b = min(stop, a + per)
            agent = self.agent[a:b, i].contiguous().to(self.device)
            index = torch.zeros(b - a, dtype=torch.int32, device=self.device)
            yield nat.render_frames(walls, goal, agent, self.size, tile_size, highlight, map_index=index)

    def frames(self, i: int, tile_size: int = 32, highlight: bool = True, start: int = 0, stop=None) -> np.ndarray:
        """The same frames on the host, uint8[k, size*ts, size*ts, 3]."""
        side = self.size * int(tile_size)
        parts = [f.cpu().numpy() for f in self.iter_frames(i, tile_size, highlight, start, stop)]
        return np.concatenate(parts) if parts else np.zeros((0, side, side, 3), dtype=np.uint8)

    def contact_sheet(self, indices=None, step="last", tile_size: int = 8, highlight: bool = True,
                      cols: int | None = None) -> np.ndarray:
        """One frame per env of `indices` (default all) tiled into one picture, uint8[rows*H, cols*W, 3]: step
        "last" is each env's final state, an int that step (clamped to the episode)."""
        idx = list(range(self.num_envs)) if indices is None else [int(i) for i in indices]
        if not idx:
            return np.zeros((0, 0, 3), dtype=np.uint8)
        at = [int(self.lengths[i]) if step == "last" else min(max(int(step), 0), int(self.lengths[i])) for i in idx]
        sel = torch.tensor(idx, dtype=torch.int64)
        agent = self.agent[torch.tensor(at), sel].contiguous().to(self.device)
        img = nat.render_frames(self.walls[sel].to(self.device), self.goal[sel].to(self.device), agent, self.size,
                                tile_size, highlight).cpu().numpy()
        k, side = len(idx), img.shape[1]
        cols = int(cols) if cols else int(np.ceil(np.sqrt(k)))
        rows = (k + cols - 1) // cols
        sheet = np.zeros((rows * side, cols * side, 3), dtype=np.uint8)
        for p in range(k):
            r, c = divmod(p, cols)
            sheet[r * side:(r + 1) * side, c * side:(c + 1) * side] = img[p]
        return sheet

    # -- files ------------------------------------------------------------------------------------------------------
    def save_npz(self, path: str) -> str:
        """The compact recording (not the pixels); Recording.load_npz reads it back."""
        meta = {"seeds": self.seeds, "difficulty": self.difficulty, "size": self.size, "max_steps": self.max_steps}
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                            walls=self.walls.numpy(), goal=self.goal.numpy(), agent=self.agent.numpy(),
                            actions=self.actions.numpy(), rewards=self.rewards.numpy(), lengths=self.lengths.numpy(),
                            returns=self.returns.numpy())
        return path if str(path).endswith(".npz") else str(path) + ".npz"

    @classmethod
    def load_npz(cls, path: str, device="cuda") -> "Recording":
        z = np.load(path, allow_pickle=False)
        meta = json.loads(bytes(z["meta"]).decode())
        return cls(meta["seeds"], meta["difficulty"], meta["size"], meta["max_steps"], z["walls"], z["goal"],
                   z["agent"], z["actions"], z["rewards"], z["lengths"], z["returns"], device=device)

    def save_gif(self, path: str, i: int, fps: int = 20, tile_size: int = 32, highlight: bool = True) -> str:
        """Env i's episode as an animated GIF, 1000 / fps ms per step.  (GIF writers fold a frame identical to the one
        before it -- a step into a wall -- into that frame's duration: the file's durations add up to the episode.)
        Without PIL the compact recording is written beside `path` instead (save_npz).  Returns the file written."""
        try:
            from PIL import Image
        except ImportError:
            alt = str(path).rsplit(".", 1)[0] + ".npz"
            print(f"PIL is not installed: wrote the compact recording {alt} instead of {path} "
                  "(Recording.load_npz(...).save_gif(...) renders it where PIL is)")
            return self.save_npz(alt)
        images = []
        for chunk in self.iter_frames(i, tile_size, highlight):
            images += [Image.fromarray(f) for f in chunk.cpu().numpy()]
        images[0].save(path, save_all=True, append_images=images[1:], duration=max(1, round(1000 / max(1, int(fps)))),
                       loop=0)
        return str(path)


def record_episodes(ac, seeds, difficulty="mediumhard", size: int = 16, device="cuda", max_steps: int | None = None,
                    **env_flags) -> Recording:
    """One deterministic episode per seed with policy `ac` (evaluate_seeds), recorded: the evaluator's actions replayed
    step by step (Recording.from_actions).  The replay must reproduce the evaluator's episode lengths and returns."""
    seeds = [int(s) for s in seeds]
    rew, steps, actions = evaluate_seeds(ac, seeds, difficulty=difficulty, size=size, device=device,
                                         max_steps=max_steps, record=True, **env_flags)
    rec = Recording.from_actions(seeds, actions, difficulty=difficulty, size=size, max_steps=max_steps, device=device,
                                 **env_flags)
    if rec.lengths.tolist() != list(steps) or rec.returns.tolist() != list(rew):
        raise RuntimeError("record_episodes: the replay of the recorded actions did not reproduce the evaluation")
    return rec
