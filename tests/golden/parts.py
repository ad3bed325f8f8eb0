"""A fixture too large for one committed file (1 MiB), stored as several: NAME.part00.npz, NAME.part01.npz, ...

save_parts(stem, arrays) packs the arrays, in order, into parts of at most PART_BYTES of array data each; an array
larger than that is cut into flat chunks `key::0`, `key::1`, ... with its shape under `key::shape`.  load_parts(stem)
puts them together again: {key: array}, bit for bit what was saved."""
from __future__ import annotations

import glob

import numpy as np

PART_BYTES = 960 << 10


def part_files(stem):
    return sorted(glob.glob(glob.escape(stem) + ".part[0-9][0-9].npz"))


def save_parts(stem, arrays):
    import os

    for f in part_files(stem):
        os.remove(f)
    pieces = []
    for key, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes > PART_BYTES:
            chunks = np.array_split(a.reshape(-1), -(-a.nbytes // PART_BYTES))
            pieces += [(f"{key}::{j}", c) for j, c in enumerate(chunks)]
            pieces.append((f"{key}::shape", np.array(a.shape, dtype=np.int64)))
        else:
            pieces.append((key, a))
    parts, size = [{}], 0
    for key, a in pieces:
        if parts[-1] and size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += a.nbytes
    for i, p in enumerate(parts):
        np.savez_compressed(f"{stem}.part{i:02d}.npz", **p)
    return len(parts)


def load_parts(stem):
    files = part_files(stem)
    if not files:
        raise FileNotFoundError(stem + ".part00.npz")
    raw = {}
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            raw.update({k: z[k] for k in z.files})
    out = {}
    for key, a in raw.items():
        base, sep, tail = key.rpartition("::")
        if not sep:
            out[key] = a
        elif tail == "shape":
            n = sum(1 for k in raw if k.startswith(base + "::")) - 1
            out[base] = np.concatenate([raw[f"{base}::{j}"] for j in range(n)]).reshape(tuple(a))
    return out
