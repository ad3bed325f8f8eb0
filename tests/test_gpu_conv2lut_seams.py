"""GPU: the conv2 table kernels (csrc/merlin_conv2lut.hip) and the conv3 glue (csrc/merlin_tower.hip: k_im2col3_fwd,
k_col2im3_bwd, k_col2im3_bwd_chunked) held to exact restatements at their seams.

The histogram backward promises exact, order-independent sums of terms rounded to 2^-K, so it is compared bit
for bit with tests/lut_hist_ref.py (vetted on the CPU by tests/test_lut_hist_ref.py), then against a float64
histogram within the bound its two roundings allow, then against the invariant that every output position reads
exactly one row of each tap.  The forward is pure float32 adds in tap order, so it is compared bit for bit with
those adds.  The grouped entry points are compared bit for bit with the ungrouped kernels on each group's slice."""
import numpy as np
import pytest
import torch

import lut_hist_ref as R
from test_conv2_tables import lut2_rows
from test_gpu_conv2lut import _codes

pytestmark = pytest.mark.gpu

INF_BITS = 0x7f800000


def _concentrated(device, n, cls):
    """Every frame the same observation: all 49 cells class cls, cell 45 class 4 (what real batches of mostly empty
    floor look like to the histogram: each tap's 25 positions fall into very few rows)."""
    from test_gpu_obs_gae import pack

    one = np.full((1, 49), cls, dtype=np.uint8)
    one[:, 45] = 4
    rows = torch.from_numpy(lut2_rows(one)).to(device).reshape(25, 16).repeat(n, 1)
    return rows, torch.from_numpy(pack(one)).to(device).repeat(n, 1).contiguous()


def _uniform(device, n, seed):
    c49, codes = _codes(device, n, seed)
    return torch.from_numpy(lut2_rows(c49)).to(device).reshape(n * 25, 16), codes


def _bits(x: float, device):
    return torch.tensor([x], dtype=torch.float32).view(torch.int32).to(device)


def _chunked(g):
    T, m, _ = g.shape
    return g.view(T, m, 16, 4).permute(0, 2, 1, 3).contiguous()


def _wide(device, T, n, seed, scale=1.0, binades=45):
    """Gradients with ReLU-style zeros and 45 binades of dynamic range below their maximum, so that a good part
    of them has bits below 2^-K (rounded, or rounded away entirely) and the rest is exact in fixed point."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    g = torch.randn(T, n * 25, 64, generator=gen)
    g[g.abs() < 0.3] = 0.0
    g = g * torch.exp2(-torch.randint(0, binades, g.shape, generator=gen).float()) * scale
    return g.to(device)


def _plant_ties(g, K):
    """Exact ties of both signs, both float32 neighbours of one, and the largest values that round to zero."""
    u = 2.0 ** -K
    v = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 4097.5, 0.25, -0.25], dtype=torch.float32) * u
    half = torch.tensor([0.5], dtype=torch.float32) * u
    v = torch.cat([v, torch.nextafter(half, half * 0), torch.nextafter(half, half * 2), -torch.nextafter(half, half * 0)])
    g[-1, : v.numel(), 5] = v.to(g.device)
    return g


def _check_hist(nat, codes, rows, g, M, n, ref_device=None):
    """dT of the kernel for gradients g (position-major) and bound M: bit-equal to the restatement, inside the
    rounding bound of the float64 histogram, and conserving every tap's column sum.  Returns (dT, ref64, count)."""
    dT = nat.conv2_lut_bwd(codes, _chunked(g), _bits(M, g.device))
    K = R.fixed_exp(M, n)
    rd = ref_device or g.device
    rows_r, g_r, dT_r = rows.to(rd), g.to(rd), dT.to(rd)
    want = R.fold(R.hist(rows_r, g_r, M, n), K)
    nbad = (dT_r.view(torch.int32) != want.view(torch.int32)).sum().item()
    assert torch.equal(dT_r, want), f"{nbad} bins differ from the fixed-point restatement (K = {K})"
    # accuracy: count terms, each within 2^-(K+1) of its value, then one float32 rounding
    ref, count = R.hist64(rows_r, g_r)
    err = (dT_r.double() - ref).abs()
    tol = R.tolerance(ref, count, K)
    assert (err <= tol).all(), (err - tol).max().item()
    assert not dT_r[count == 0].any()
    # invariant: every output position reads exactly one row of each tap
    d64, col = dT_r.double(), g_r.double().sum(1)
    for k in range(16):
        rr = list(R.tap_row_range(k))
        bins = d64[:, rr]
        assert ((bins.sum(1) - col).abs() <= 2.0 ** -24 * bins.abs().sum(1)).all(), k
    db2 = d64[:, 0:20:4].sum(1)  # what _GroupedConv2LutTower.backward returns as the conv2 bias gradient
    assert ((db2 - col).abs() <= 2.0 ** -24 * d64[:, 0:20:4].abs().sum(1)).all()
    return dT_r, ref, count


# ---------------------------------------------------------------------------------------------------------------
# histogram
# 1 | 3 | 4 | 5: a wave's group of 4 frames; 63 | 64 | 65: the 16 waves' first trip and a second trip through the
# prefetch loop; 256 | 257, 1792 | 1793: one more frame block; 2049: the cap at 8 blocks, `per` rounded up to 260
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 256, 257, 1792, 1793, 2049])
def test_histogram_frame_seams_bitwise(device, n):
    from merlin import _native as nat

    rows, codes = _uniform(device, n, seed=500 + n)
    g = _wide(device, 2, n, seed=n)
    M = g.abs().max().item()
    g = _plant_ties(g, R.fixed_exp(M, n))
    _check_hist(nat, codes, rows, g, M, n)


@pytest.mark.parametrize("n,cls", [(1310, 1), (1311, 2)])
def test_histogram_concentrated_bitwise(device, n, cls):
    """25 n + 1 crosses 2^15 between the two: the rows of a concentrated batch receive up to 25 n terms of the full
    magnitude, which is what the overflow headroom 62 - lg - e is for."""
    from merlin import _native as nat

    M = 0.75
    rows, codes = _concentrated(device, n, cls)
    g = torch.full((2, n * 25, 64), M, device=device)
    dT, _, count = _check_hist(nat, codes, rows, g, M, n)
    assert torch.equal(dT.double(), count.double() * M)
    assert count.max().item() >= 20 * n  # concentrated indeed


def test_histogram_concentrated_at_the_power_of_two(device):
    """n = 41,943: 25 n + 1 = 2^20, the one n where the lg loop's comparison is decided by equality.  All terms
    +0.75 with the bound exactly 0.75: every touched bin is count * 0.75 exactly.  K = 42 and K = 41 both hold such
    terms exactly, so a second pass over the same frames uses terms of 3 * 2^-42 under the same (now loose) bound:
    exact at K = 42, a tie at K = 41."""
    from merlin import _native as nat

    n, M = 41943, 0.75
    assert R.fixed_exp(M, n) == 42
    rows, codes = _concentrated(device, n, 1)
    g = torch.full((1, n * 25, 64), M, device=device)
    dT, _, count = _check_hist(nat, codes, rows, g, M, n)
    assert torch.equal(dT.double(), count.double() * M)
    small = 3 * 2.0 ** -42
    g.fill_(small)
    dT = nat.conv2_lut_bwd(codes, _chunked(g), _bits(M, device))
    assert torch.equal(dT.double(), count.double() * small)


@pytest.mark.parametrize("case", ["loose_1024x", "power_of_two_max", "all_zero", "scaled_down", "scaled_up"])
def test_histogram_absmax_cases(device, case):
    from merlin import _native as nat

    n = 300
    rows, codes = _uniform(device, n, seed=77)
    if case == "all_zero":
        g = torch.zeros(2, n * 25, 64, device=device)
        dT, _, _ = _check_hist(nat, codes, rows, g, 0.0, n)
        assert not dT.any() and not torch.isnan(dT).any()
        return
    if case == "scaled_down":
        # no spread here: non-zero terms of at least 0.3 * 2^-100 are multiples of 2^-125, and so are their sums,
        # so neither an input nor a result is subnormal (test_histogram_denormal_gradients has those)
        g = _wide(device, 2, n, seed=78, scale=2.0 ** -100, binades=1)
        M = g.abs().max().item()
        _check_hist(nat, codes, rows, g, M, n)
        return
    g = _wide(device, 2, n, seed=78, scale=2.0 ** 100 if case == "scaled_up" else 1.0)
    if case == "power_of_two_max":  # the bound 2^e' is attained: e must be e' + 1, not e'
        g.clamp_(-4.0, 4.0)
        g[1, 7, 3] = -4.0
    M = g.abs().max().item()
    if case == "power_of_two_max":
        assert M == 4.0
    if case == "loose_1024x":  # an upper bound is all the contract asks of absmax
        M *= 1024.0
    _check_hist(nat, codes, rows, _plant_ties(g, R.fixed_exp(M, n)), M, n)


def test_histogram_denormal_gradients(device):
    """Subnormal float32 inputs (the E == 0 branch of the kernel's bit formula).  The gradients are positive and
    drawn from [2^-135, 2^-121] on concentrated frames at n = 128, so every touched bin sums 3,200 terms of at
    least 2^-135 and is a normal float: the assertion does not rest on how the device stores a subnormal result.
    The restatement runs on the CPU for the same reason (its float32 -> float64 conversion must not flush)."""
    from merlin import _native as nat

    n, M = 128, 2.0 ** -120
    rows, codes = _concentrated(device, n, 1)
    rs = np.random.RandomState(5)
    g64 = 2.0 ** (-135 + 14 * rs.rand(2, n * 25, 64))
    g_cpu = torch.from_numpy(g64.astype(np.float32))
    assert g_cpu.min().item() >= 2.0 ** -135 and (g_cpu < 2.0 ** -126).float().mean().item() > 0.5
    g = g_cpu.to(device)
    assert torch.equal(g.cpu().view(torch.int32), g_cpu.view(torch.int32))
    dT, ref, count = _check_hist(nat, codes, rows, g, M, n, ref_device=torch.device("cpu"))
    assert (dT[count > 0] >= 2.0 ** -126).all() and (count[count > 0] % 128 == 0).all()


def test_histogram_non_finite_bound(device):
    from merlin import _native as nat

    n = 5
    _, codes = _uniform(device, n, seed=9)
    g = _wide(device, 2, n, seed=9)
    dT = nat.conv2_lut_bwd(codes, _chunked(g), torch.tensor([INF_BITS], dtype=torch.int32, device=device))
    assert torch.isnan(dT).all()
    # a NaN gradient reaches the histogram as a bound of +inf and leaves it as NaN.  The NaN sits at frame 0,
    # position 0, channel 0: the first of the three outputs its thread computes, so the bound has to survive the
    # finite values that follow it
    gen = torch.Generator(device="cpu").manual_seed(3)
    dA3 = torch.randn(2, n * 9, 576, generator=gen).to(device)
    Z2 = torch.randn(2, n * 25, 64, generator=gen).to(device)
    b2 = torch.randn(2, 64, generator=gen).to(device)
    for t, s, p3, tap, ci in ((0, 0, 0, 0, 0), (1, 4, 8, 8, 63)):
        bad = dA3.clone()
        bad[t, s * 9 + p3, tap * 64 + ci] = float("nan")
        z = Z2.clone()
        p2 = (p3 // 3 + tap // 3) * 5 + p3 % 3 + tap % 3
        z[t, s * 25 + p2, ci] = 1.0 - b2[t, ci]  # kept by the ReLU mask
        dZ2c, absmax = nat.conv3_col2im_bwd_chunked(bad, z, b2)
        assert torch.isnan(dZ2c[t, ci // 4, s * 25 + p2, ci % 4])
        assert absmax.item() == INF_BITS, hex(absmax.item())
        assert torch.isnan(nat.conv2_lut_bwd(codes, dZ2c, absmax)).all()
    # and an infinite gradient likewise
    bad = dA3.clone()
    bad[1, 2 * 9 + 4, 4 * 64 + 9] = float("-inf")
    z = Z2.clone()
    z[1, 2 * 25 + 12, 9] = 1.0 - b2[1, 9]
    dZ2c, absmax = nat.conv3_col2im_bwd_chunked(bad, z, b2)
    assert absmax.item() == INF_BITS
    assert torch.isnan(nat.conv2_lut_bwd(codes, dZ2c, absmax)).all()


# ---------------------------------------------------------------------------------------------------------------
# grouped against ungrouped
def _grouped_case(device, G, F, seed):
    """Codes, tables and gradients of G groups of F frames; group g's tables and gradients are scaled by 2^(3g), so
    a row read from, or credited to, the neighbouring group cannot pass.  The codes are the head of a pool twice
    as long: a group offset that is wrong by up to a factor of two still reads defined rows and fails by value."""
    _, pool = _codes(device, 2 * G * F, seed)
    codes = pool[: G * F]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    scale = torch.exp2(3.0 * torch.arange(G).repeat_interleave(2).float()).view(2 * G, 1, 1)
    T2 = (torch.randn(2 * G, 2720, 64, generator=gen) * scale).to(device)
    g = torch.randn(2 * G, F * 25, 64, generator=gen)
    g[g.abs() < 0.3] = 0.0
    g = (g * torch.exp2(-torch.randint(0, 45, g.shape, generator=gen).float()) * scale).to(device)
    return codes, T2, g


def _check_grouped_bwd(nat, device, G, F, seed):
    codes, _, g = _grouped_case(device, G, F, seed)
    dZ2c = _chunked(g)
    absmax = _bits(g.abs().max().item(), device)  # one word for every group, as col2im3 produces it
    dT = nat.conv2_lut_bwd_grouped(codes, dZ2c, absmax)
    assert dT.shape == (2 * G, 2720, 64)
    for gi in range(G):
        want = nat.conv2_lut_bwd(codes[gi * F:(gi + 1) * F], dZ2c[2 * gi:2 * gi + 2], absmax)
        assert torch.equal(dT[2 * gi:2 * gi + 2], want), (G, F, gi)
        assert want.any()


# F = 2, 3: a wave's group of 4 frames spans three or four tasks; F = 257: two frame blocks per slice
@pytest.mark.parametrize("F", [1, 2, 3, 5, 37, 257])
@pytest.mark.parametrize("G", [1, 3, 5])
def test_grouped_forward_matches_ungrouped_bitwise(device, G, F):
    from merlin import _native as nat

    codes, T2, _ = _grouped_case(device, G, F, seed=1000 * G + F)
    Z2 = nat.conv2_lut_fwd_grouped(codes, T2, F)
    assert Z2.shape == (2 * G, F * 25, 64)
    for gi in range(G):
        want = nat.conv2_lut_fwd(codes[gi * F:(gi + 1) * F], None, T2[2 * gi:2 * gi + 2])
        assert torch.equal(Z2[2 * gi:2 * gi + 2], want), (G, F, gi)


@pytest.mark.parametrize("F", [1, 2, 3, 5, 37, 257])
@pytest.mark.parametrize("G", [1, 3, 5])
def test_grouped_backward_matches_ungrouped_bitwise(device, G, F):
    from merlin import _native as nat

    _check_grouped_bwd(nat, device, G, F, seed=2000 * G + F)


def test_grouped_backward_slab_buffer_shrinks_in_use(device):
    """The Python-side slab buffer is kept at its largest size: after (G, F) = (5, 257) it holds 2 x 5 x 16 x 2
    slabs of which (1, 1) uses the first 32.  Stale slabs must not leak into the smaller call."""
    from merlin import _native as nat

    assert nat.lib().merlin_tower_conv2_lut_slab_bytes(10, 257) == 8 * 10 * 16 * 2 * 2720 * 4
    assert nat.lib().merlin_tower_conv2_lut_slab_bytes(2, 1) == 8 * 2 * 16 * 1 * 2720 * 4
    assert nat.lib().merlin_tower_conv2_lut_slab_bytes(2, 10 ** 6) == 8 * 2 * 16 * 8 * 2720 * 4
    _check_grouped_bwd(nat, device, 5, 257, seed=31)
    _check_grouped_bwd(nat, device, 1, 1, seed=32)


# ---------------------------------------------------------------------------------------------------------------
# forward
def _in_order_sum(tab, rows):
    """acc = T[r0]; acc += T[r1]; ... in float32 and tap order; tab [2720, 64], rows [m, 16] -> [m, 64]."""
    acc = tab[rows[:, 0]]
    for k in range(1, 16):
        acc = acc + tab[rows[:, k]]
    return acc


@pytest.mark.parametrize("use_index", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 333])
@pytest.mark.parametrize("T", [1, 2])
def test_forward_is_the_in_order_sum(device, T, n, use_index):
    from merlin import _native as nat

    pool = max(n, 40)
    c49, codes = _codes(device, pool, seed=300 + n)
    gen = torch.Generator(device="cpu").manual_seed(n + T)
    T2 = torch.randn(T, 2720, 64, generator=gen).to(device)
    idx = torch.randint(0, pool, (n,), generator=gen).to(device) if use_index else None
    sel = idx.cpu().numpy() if use_index else np.arange(n)
    rows = torch.from_numpy(lut2_rows(c49[sel])).to(device).reshape(n * 25, 16)
    Z2 = nat.conv2_lut_fwd(codes if use_index else codes[:n], idx, T2)
    assert Z2.shape == (T, n * 25, 64)
    for t in range(T):
        # pure adds and -ffp-contract=off: the equality is owed
        assert torch.equal(Z2[t], _in_order_sum(T2[t], rows)), t
        picked = T2[t].double()[rows]  # [m, 16, 64]
        err = (Z2[t].double() - picked.sum(1)).abs()
        assert (err <= 15 * 2.0 ** -24 * picked.abs().sum(1)).all()


@pytest.mark.parametrize("use_index", [False, True])
def test_forward_grid_stride(device, use_index):
    """n = 32,771 frames are 8,193 wave groups, one more than the 2,048 blocks x 4 waves of the capped grid take in
    one trip.  The whole result equals the kernel's own results on three pieces that do not stride, and 1,024
    sampled frames (the last three among them) equal the in-order sum."""
    from merlin import _native as nat

    n = 32771
    c49, codes = _codes(device, n, seed=41)
    gen = torch.Generator(device="cpu").manual_seed(41)
    T2 = torch.randn(1, 2720, 64, generator=gen).to(device)
    idx = torch.randint(0, n, (n,), generator=gen).to(device) if use_index else None
    Z2 = nat.conv2_lut_fwd(codes, idx, T2)
    cuts = [0, 16384, 32768, n]
    pieces = [nat.conv2_lut_fwd(codes, idx[a:b].contiguous(), T2) if use_index else
              nat.conv2_lut_fwd(codes[a:b], None, T2) for a, b in zip(cuts, cuts[1:])]
    assert torch.equal(Z2, torch.cat(pieces, dim=1))
    frames = np.unique(np.concatenate([np.random.RandomState(1).randint(0, n, size=1021), [n - 3, n - 2, n - 1]]))
    sel = idx.cpu().numpy()[frames] if use_index else frames
    rows = torch.from_numpy(lut2_rows(c49[sel])).to(device).reshape(-1, 16)
    got = Z2[0].view(n, 25, 64)[torch.from_numpy(frames).to(device)].reshape(-1, 64)
    assert torch.equal(got, _in_order_sum(T2[0], rows))


# ---------------------------------------------------------------------------------------------------------------
# conv3 glue
def _unfold3(H, T, n):
    """[T, n*25, 64] -> [T, n*9, 576]: A3[t][s*9 + oy*3 + ox][(ky*3 + kx)*64 + ci] = H[t][s*25 + (oy+ky)*5 + ox+kx][ci]"""
    w = H.view(T, n, 5, 5, 64).unfold(2, 3, 1).unfold(3, 3, 1)  # [T, n, oy, ox, ci, ky, kx]
    return w.permute(0, 1, 2, 3, 5, 6, 4).reshape(T, n * 9, 576)


def _col2im64(dA3, T, n):
    X = torch.zeros(T, n * 25, 64, dtype=torch.float64, device=dA3.device, requires_grad=True)
    _unfold3(X, T, n).backward(dA3.double())
    return X.grad


# 2 x ceil(4099 / 2) = 4,100 and 6 x ceil(1501 / 2) = 4,506 blocks' worth of work: past the cap of 4,096 of all three
@pytest.mark.parametrize("T,n", [(2, 4099), (6, 1501)])
def test_conv3_glue_past_the_grid_cap(device, T, n):
    from merlin import _native as nat

    gen = torch.Generator(device="cpu").manual_seed(T * n)
    Z2 = torch.randn(T, n * 25, 64, generator=gen).to(device)
    b2 = torch.randn(T, 64, generator=gen).to(device)
    dA3 = torch.randn(T, n * 9, 576, generator=gen).to(device)
    dA3[T - 1] *= 2.0  # the largest |dZ2| then sits in the last tower: the bound is over all of them
    # Z2 = -b2 exactly: Z2 + b2 == 0 counts as masked (first, middle and last frame of every tower)
    planted = [(t, s * 25 + p, c) for t in range(T) for s, p, c in ((0, 0, 0), (n // 2, 12, 31), (n - 1, 24, 63))]
    for t, r, c in planted:
        Z2[t, r, c] = -b2[t, c]

    pre = Z2 + b2[:, None, :]
    assert torch.equal(nat.conv3_im2col_fwd(Z2, b2), _unfold3(torch.relu(pre), T, n))

    flat = nat.conv3_col2im_bwd(dA3, Z2, b2)
    keep = pre > 0
    for t, r, c in planted:
        assert not keep[t, r, c] and flat[t, r, c] == 0
    assert not flat[~keep].any()  # the mask is exact
    ref = _col2im64(dA3, T, n)
    mag = _col2im64(dA3.abs(), T, n)  # each output sums at most 9 terms: 8 float32 adds
    assert ((flat.double() - ref).abs()[keep] <= (8 * 2.0 ** -24 * mag)[keep]).all()
    assert (ref[keep] != 0).all()  # so the zeros above are the mask's doing

    ch, absmax = nat.conv3_col2im_bwd_chunked(dA3, Z2, b2)
    assert ch.shape == (T, 16, n * 25, 4)
    assert torch.equal(ch.permute(0, 2, 1, 3).reshape(T, n * 25, 64), flat)
    amax = flat.abs().max()
    assert absmax.view(torch.float32).item() == amax.item()
    assert flat[T - 1].abs().max() == amax and flat[: T - 1].abs().max() < amax
