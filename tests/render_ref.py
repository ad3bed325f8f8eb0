"""TEST INFRASTRUCTURE ONLY -- the checker of the full-grid renderer: minigrid 3.0.0's get_frame(highlight,
tile_size) = get_full_render restated in plain Python from the two restatements the suite already pins the library
to, oracle/tiles.py (render_tile) and oracle/minigrid_literal.py (Grid.slice / rotate_left / process_vis).

    get_full_render:  _, vis_mask = gen_obs_grid()                       # slice, rotate_left x (dir + 1), process_vis
                      f_vec, r_vec = dir_vec, right_vec
                      top_left = agent_pos + f_vec * (view - 1) - r_vec * (view // 2)
                      for vis_j, vis_i: if vis_mask[vis_i, vis_j]:
                          abs = top_left - f_vec * vis_j + r_vec * vis_i;  skip outside the grid
                          highlight_mask[abs] = True
                      Grid.render(tile_size, agent_pos, agent_dir, highlight_mask)
    Grid.render:      tile (i, j) = render_tile(cell, agent_dir if agent_pos == (i, j) else None,
                                                highlight_mask[i, j], tile_size) -> img[ts j : ts j + ts, ts i : ts i + ts]

minigrid itself is not installed: like the two modules it is built from, this is a restatement ("parity unpinned"
with respect to minigrid itself).
"""
from __future__ import annotations

import numpy as np

import minigrid_literal as ML
import tiles

VIEW = 7
_TILES: dict = {}


def tile(obj, agent_dir, highlight, tile_size):
    """render_tile(obj, agent_dir, highlight, tile_size), computed once per key."""
    key = (obj, agent_dir, bool(highlight), int(tile_size))
    if key not in _TILES:
        _TILES[key] = tiles.render_tile(obj, agent_dir, bool(highlight), int(tile_size))
    return _TILES[key]


def grid_of(cells, goal):
    """An ML.Grid from cells uint8[size][size] ([y][x], 1 = wall) and the goal's (x, y) or None."""
    S = len(cells)
    g = ML.Grid(S, S)
    for y in range(S):
        for x in range(S):
            if int(cells[y][x]) == 1:
                g.set(x, y, ML.WALL)
    if goal is not None and 0 <= goal[0] < S and 0 <= goal[1] < S and g.get(int(goal[0]), int(goal[1])) is None:
        g.set(int(goal[0]), int(goal[1]), ML.GOAL)
    return g


def cells_of_rows(rows, size):
    """uint8[size][size] wall cells from bit rows (bit x of rows[y] = wall at (x, y))."""
    rows = np.asarray(rows).astype(np.uint32)
    return ((rows[:size, None] >> np.arange(size, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)


def highlight_mask(grid, agent_pos, agent_dir):
    """(mask bool[size][size] indexed [i][j], view cells that fell outside the grid, in-grid window cells left dark)."""
    ax, ay = int(agent_pos[0]), int(agent_pos[1])
    d = int(agent_dir)
    v = VIEW
    if d == 0:
        tx, ty = ax, ay - v // 2
    elif d == 1:
        tx, ty = ax - v // 2, ay
    elif d == 2:
        tx, ty = ax - v + 1, ay - v // 2
    else:
        tx, ty = ax - v // 2, ay - v + 1
    g = grid.slice(tx, ty, v, v)
    for _ in range(d + 1):
        g = g.rotate_left()
    vis = g.process_vis(agent_pos=(v // 2, v - 1))
    f = ML.DIR_TO_VEC[d]
    r = (-f[1], f[0])
    top_left = (ax + f[0] * (v - 1) - r[0] * (v // 2), ay + f[1] * (v - 1) - r[1] * (v // 2))
    mask = np.zeros((grid.width, grid.height), dtype=bool)
    outside = dark = 0
    for vis_j in range(v):
        for vis_i in range(v):
            abs_i = top_left[0] - f[0] * vis_j + r[0] * vis_i
            abs_j = top_left[1] - f[1] * vis_j + r[1] * vis_i
            inside = 0 <= abs_i < grid.width and 0 <= abs_j < grid.height
            if not inside:
                outside += 1
            elif not vis[vis_i, vis_j]:
                dark += 1
            if not vis[vis_i, vis_j] or not inside:
                continue
            mask[abs_i, abs_j] = True
    return mask, outside, dark


def full_render(cells, goal, agent_pos, agent_dir, tile_size=32, highlight=True, info=None):
    """uint8[size*ts, size*ts, 3].  info (a dict, optional) receives 'outside' (view cells outside the grid) and
    'dark' (cells of the grid inside the view window that are not visible)."""
    grid = grid_of(cells, goal)
    S, ts = grid.width, int(tile_size)
    mask, outside, dark = highlight_mask(grid, agent_pos, agent_dir)
    if info is not None:
        info["outside"], info["dark"] = outside, dark
    img = np.zeros((S * ts, S * ts, 3), dtype=np.uint8)
    for j in range(S):
        for i in range(S):
            here = (i, j) == (int(agent_pos[0]), int(agent_pos[1]))
            t = tile(grid.get(i, j), int(agent_dir) if here else None, bool(highlight) and bool(mask[i, j]), ts)
            img[j * ts:(j + 1) * ts, i * ts:(i + 1) * ts] = t
    return img
