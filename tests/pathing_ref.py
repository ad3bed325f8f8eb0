"""The path tests' own reference (no test in here): a forward breadth-first search over (x, y, dir) written from the
step rule -- 0 turn left (dir + 3) & 3, 1 turn right (dir + 1) & 3, 2 forward into a non-wall cell, terminating on the
forward action whose front cell is the goal; directions 0 = +x, 1 = +y, 2 = -x, 3 = -y.  It shares no code with the
library: the kernel and the library's host restatement both search backwards from the goal."""
from collections import deque

import numpy as np

from test_gpu_env_sizes import MATRIX, P_FWD  # noqa: F401  (the size matrix every path test runs over)

CASES = [(d, s) for d, sizes in MATRIX.items() for s in sizes]
IDS = [f"{d}-{s}" for d, s in CASES]
SEED0, N = 1000, 130


def bfs(cells, pos, direction, goal):
    """Least number of actions after which an episode started at pos = (x, y), direction, terminates; -1 if none
    does.  cells[y][x] == 1 is a wall (MerlinVecEnv.get_state()["cells"] / oracle.gen_map)."""
    S = cells.shape[0]
    gx, gy = int(goal[0]), int(goal[1])
    start = (int(pos[0]), int(pos[1]), int(direction))
    seen, queue = {start: 0}, deque([start])
    while queue:
        x, y, d = p = queue.popleft()
        fx, fy = x + (1, 0, -1, 0)[d], y + (0, 1, 0, -1)[d]
        if (fx, fy) == (gx, gy):
            return seen[p] + 1  # forward terminates here
        nxt = [(x, y, (d + 3) & 3), (x, y, (d + 1) & 3)]
        if 0 <= fx < S and 0 <= fy < S and cells[fy][fx] != 1:
            nxt.append((fx, fy, d))
        for s in nxt:
            if s not in seen:
                seen[s] = seen[p] + 1
                queue.append(s)
    return -1


def bfs_state(st, idx):
    """bfs of the envs idx of a get_state() dict."""
    return np.array([bfs(st["cells"][i], st["agent_pos"][i], st["agent_dir"][i], st["goal_pos"][i]) for i in idx],
                    dtype=np.int32)


def oracle_maps(oracle, diff, size, seeds):
    """(cells uint8[n, S, S], walls uint32[n, S] bit rows, goal int32[n, 2], agent int32[n, 4]) of oracle.gen_map."""
    cells, goal, agent = [], [], []
    for s in seeds:
        c, meta = oracle.gen_map(size, diff, int(s))
        cells.append(c)
        agent.append((meta[0], meta[1], meta[2], 0))
        goal.append((meta[3], meta[4]))
    cells = np.stack(cells)
    walls = ((cells == 1).astype(np.uint64) << np.arange(size, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return cells, walls, np.array(goal, dtype=np.int32), np.array(agent, dtype=np.int32)
