"""Mixtures of difficulties for one vector env: ``"easy:1,mediumhard:2,hard:1"`` -> per-env names.

``assign`` lays the classes out as contiguous runs in the order easy, medium, mediumhard, hard, hardest, with run
boundaries on multiples of ``align`` envs (64: one wavefront of the env kernels), so that every wave of the full-width
reset / refill passes runs one generator (one lane generates one env's map; a wave holding several classes runs their
generators one after another -- csrc/merlin_env.hip env_difficulty).
"""
from __future__ import annotations

DIFFICULTIES = ("easy", "medium", "mediumhard", "hard", "hardest")


def parse_mix(spec) -> dict:
    """``"name:w,name:w"`` (or a dict) -> {name: float weight}, in the order given.  A bare name weighs 1.
    Unknown names, repeated names and weights that are not positive raise ValueError."""
    if isinstance(spec, dict):
        items = list(spec.items())
    else:
        items = []
        for part in str(spec).split(","):
            part = part.strip()
            if not part:
                continue
            name, _, w = part.partition(":")
            items.append((name.strip(), w.strip() if w.strip() else "1"))
    if not items:
        raise ValueError(f"empty difficulty mix: {spec!r}")
    out = {}
    for name, w in items:
        if name not in DIFFICULTIES:
            raise ValueError(f"Unknown difficulty: {name}")
        if name in out:
            raise ValueError(f"difficulty {name} given twice in the mix")
        try:
            w = float(w)
        except (TypeError, ValueError):
            raise ValueError(f"weight of {name} is not a number: {w!r}") from None
        if not (w > 0.0) or w == float("inf"):
            raise ValueError(f"weight of {name} must be positive and finite, got {w}")
        out[name] = w
    return out


def format_mix(weights: dict) -> str:
    """The inverse of parse_mix: ``parse_mix(format_mix(w)) == w``."""
    return ",".join(f"{name}:{float(w)!r}" for name, w in weights.items())


def is_mix(spec) -> bool:
    """A dict, or a string in the ``name:w,...`` form (a plain difficulty name is not a mix)."""
    return isinstance(spec, dict) or (isinstance(spec, str) and ("," in spec or ":" in spec))


def _largest_remainder(units: int, weights: list) -> list:
    """`units` split in proportion to the weights (units >= len(weights)): the floors of the exact quotas, the
    left-over units to the largest remainders (ties: the earlier class); then every class left with nothing takes one
    unit from the class that holds the most (ties: the earlier class)."""
    k = len(weights)
    total = sum(weights)
    quota = [units * w / total for w in weights]
    share = [int(q) for q in quota]
    order = sorted(range(k), key=lambda j: (-(quota[j] - share[j]), j))
    for j in order[:max(0, units - sum(share))]:
        share[j] += 1
    while sum(share) > units:  # a quota rounded up to the next integer in floating point
        share[max(range(k), key=lambda i: (share[i], -i))] -= 1
    for j in range(k):
        if share[j] == 0:
            big = max(range(k), key=lambda i: (share[i], -i))
            share[big] -= 1
            share[j] = 1
    return share


def assign(num_envs: int, weights, align: int = 64) -> list:
    """Per-env difficulty names for `num_envs` envs: contiguous runs in the order of DIFFICULTIES, sized by largest
    remainder on units of `align` envs (the last unit may be partial: it goes to the last class); units of 1 when
    num_envs < align * classes.  Every class with a positive weight gets at least one env.  Deterministic."""
    weights = parse_mix(weights)
    names = [d for d in DIFFICULTIES if d in weights]
    num_envs, align = int(num_envs), max(1, int(align))
    if num_envs < len(names):
        raise ValueError(f"{num_envs} envs cannot hold {len(names)} difficulties")
    unit = align if num_envs >= align * len(names) else 1
    units = (num_envs + unit - 1) // unit
    share = _largest_remainder(units, [weights[d] for d in names])
    out = []
    for d, s in zip(names, share):
        out += [d] * (s * unit)
    return out[:num_envs]
