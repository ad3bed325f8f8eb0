"""The conv2 table histogram (csrc/merlin_conv2lut.hip: k_conv2_lut_hist + k_conv2_lut_fold) restated in
plain torch ops, on either device.  It restates what the file's header promises, not how the kernel does it:

    dT[t][row] = (sum over the (frame, position, tap) triples whose tap reads `row` of round(g * 2^K)) * 2^-K

with every term rounded to the nearest multiple of 2^-K (ties away from zero), the sum taken in integers (so
its order cannot matter), and one final rounding to float32.  K = 62 - lg - e, where 2^lg >= 25 n + 1 (the
number of terms a row can receive, plus one) and absmax < 2^e, so no partial sum reaches 2^62.

tests/test_lut_hist_ref.py vets every function here against exact rational arithmetic on the CPU;
tests/test_gpu_conv2lut_seams.py holds the kernels to it bit for bit.
"""
import math

import torch

NROW, C2, P2, TAPS = 2720, 64, 25, 16


def fixed_exp(absmax: float, n: int) -> int:
    """K of the header comment.  absmax is a finite float32 value >= 0 (as a Python float), n the frames."""
    assert math.isfinite(absmax) and absmax >= 0.0 and n >= 1
    e = math.frexp(absmax)[1]        # absmax = m * 2^e with 1/2 <= m < 1, so absmax < 2^e; frexp(0) = (0, 0)
    lg = (P2 * n).bit_length()       # the smallest lg with 2^lg >= 25 n + 1
    return 62 - lg - e


def to_fixed(g: torch.Tensor, K: int) -> torch.Tensor:
    """sign(g) * floor(|g| * 2^K + 1/2) as int64.  |g| * 2^K is a float32 scaled by a power of two, exact in
    float64; its floor and the remainder x - floor(x) are exact too, so no rounding happens but the one asked for."""
    assert g.dtype == torch.float32
    x = g.double().abs() * (2.0 ** K)
    f = torch.floor(x)
    q = (f + (x - f >= 0.5).double()).to(torch.int64)
    return torch.where(g < 0, -q, q)


def _blocks(m: int) -> int:
    # the rows are added in up to 64 private copies that are summed afterwards: integer adds, so the same sum,
    # without every term of a concentrated batch queueing on the same few addresses
    return max(1, min(64, m // 1024))


def _scatter(rows: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """out[t][r] = sum of v[t][i] over the (i, k) with rows[i][k] == r; rows [m, 16], v [T, m, 64]."""
    T, m, _ = v.shape
    nb = _blocks(m)
    blk = (torch.arange(m, device=v.device) % nb) * NROW
    out = torch.zeros(T, nb * NROW, C2, dtype=v.dtype, device=v.device)
    for k in range(TAPS):
        idx = rows[:, k] + blk
        for t in range(T):
            out[t].index_add_(0, idx, v[t])
    return out.view(T, nb, NROW, C2).sum(1)


def hist(rows: torch.Tensor, g: torch.Tensor, absmax: float, n: int) -> torch.Tensor:
    """int64 [T, 2720, 64]: the fixed-point sums.  rows int64 [n*25, 16] (tests/test_conv2_tables.py::lut2_rows),
    g float32 [T, n*25, 64] (position-major, not the kernel's chunked layout)."""
    assert rows.shape == (n * P2, TAPS) and g.shape[1:] == (n * P2, C2)
    return _scatter(rows, to_fixed(g, fixed_exp(absmax, n)))


def fold(acc: torch.Tensor, K: int) -> torch.Tensor:
    """float32(ldexp(float64(acc), -K)): int64 -> float64 and float64 -> float32 both round to nearest even."""
    return (acc.double() * (2.0 ** -K)).float()


def hist64(rows: torch.Tensor, g: torch.Tensor):
    """(ref, count): the same histogram of the unrounded gradients in float64, and how many non-zero terms each
    bin received (a zero term is exact in fixed point, so only the others carry a rounding error)."""
    ref = _scatter(rows, g.double())
    count = _scatter(rows, (g != 0).to(torch.int64))
    return ref, count


def tolerance(ref: torch.Tensor, count: torch.Tensor, K: int) -> torch.Tensor:
    """The bound on |dT - ref| that follows from the two roundings: each of a bin's `count` terms is off by at
    most half a unit 2^-K, and the float32 result by at most 2^-24 of its value (2^-149 where it is subnormal)."""
    tol = 2.0 ** -24 * ref.abs() + count.double() * 2.0 ** -(K + 1)
    return tol + (ref.abs() < 2.0 ** -126).double() * 2.0 ** -149


def tap_row_range(k: int) -> range:
    """The table rows tap k = 4*ky + kx can read: its parity type's block, every fourth row from j."""
    ky, kx = k >> 2, k & 3
    lo, hi = ((0, 20), (20, 120), (120, 220), (220, NROW))[2 * (ky & 1) + (kx & 1)]
    return range(lo + 2 * (ky >> 1) + (kx >> 1), hi, 4)
