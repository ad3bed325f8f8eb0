"""GPU parity: observation expansion (bit-exact vs the oracle render of the same codes)
and GAE / advantage normalisation (vs the reference's own outputs: gae_ref.npz,
tolerance 1e-5 as north_star states; the thread-per-env kernel keeps the reference's
fp32 op order and is checked bit-exact too)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def pack(codes_u8: np.ndarray) -> np.ndarray:
    n = codes_u8.shape[0]
    nib = np.zeros((n, 64), dtype=np.uint32)
    nib[:, :49] = codes_u8
    w = (nib.reshape(n, 8, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(-1).astype(np.uint32)
    return w.view(np.int32)


@pytest.fixture(scope="module")
def codes_case():
    rs = np.random.RandomState(0)
    c = rs.randint(0, 5, size=(777, 49)).astype(np.uint8)
    c[:, 45] = 4
    return c


def test_expand_u8_matches_oracle_render(golden, oracle, device, codes_case):
    from merlin import _native as nat

    codes = torch.from_numpy(pack(codes_case)).to(device)
    out = nat.expand_obs_u8(codes).cpu().numpy()
    ref = oracle.render(codes_case, golden("atlas")["atlas"])
    assert (out == ref).all()


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_expand_f32_layouts_and_scale(golden, oracle, device, codes_case, layout):
    from merlin import _native as nat

    codes = torch.from_numpy(pack(codes_case)).to(device)
    ref = oracle.render(codes_case, golden("atlas")["atlas"]).astype(np.float32)
    if layout == "nchw":
        ref = ref.transpose(0, 3, 1, 2)
    out = nat.expand_obs(codes, layout=layout).cpu().numpy()
    assert (out == ref).all()
    out = nat.expand_obs(codes, layout=layout, scale=1.0 / 255.0).cpu().numpy()
    assert (out == ref * np.float32(1.0 / 255.0)).all()


def test_expand_gather_by_index(golden, oracle, device, codes_case):
    from merlin import _native as nat

    codes = torch.from_numpy(pack(codes_case)).to(device)
    idx = torch.randperm(777, device=device)[:300]
    out = nat.expand_obs(codes, index=idx).cpu().numpy()
    ref = oracle.render(codes_case[idx.cpu().numpy()], golden("atlas")["atlas"]).astype(np.float32)
    assert (out == ref.transpose(0, 3, 1, 2)).all()


def test_expand_empty(device):
    from merlin import _native as nat

    codes = torch.zeros((0, 8), dtype=torch.int32, device=device)
    assert nat.expand_obs(codes).shape == (0, 3, 56, 56)


def _gae(device, r, v, d, lv, gamma=0.99, lam=0.95, stats=None):
    from merlin import _native as nat

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)  # noqa: E731
    adv, ret = nat.gae(t(r), t(v), t(d), t(np.atleast_1d(lv)), gamma, lam, stats=stats)
    return adv.cpu().numpy(), ret.cpu().numpy()


def test_gae_single_env_vs_reference(golden, device):
    g = golden("gae_ref")
    for k in range(int(g["ncases"])):
        r, v, d, lv = g[f"c{k}_r"], g[f"c{k}_v"], g[f"c{k}_d"], g[f"c{k}_last"]
        adv, ret = _gae(device, r, v, d, lv)  # N=1: the wave-scan kernel
        np.testing.assert_allclose(adv, g[f"c{k}_adv"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(ret, g[f"c{k}_ret"], rtol=1e-5, atol=1e-5)
        adv, ret = _gae(device, r, v, d, lv, gamma=0.995)  # compute_gae_standard (FOMAML gamma)
        np.testing.assert_allclose(adv, g[f"c{k}_adv995"], rtol=1e-5, atol=1e-5)


def test_gae_thread_kernel_bit_exact_with_reference_order(golden, oracle, device):
    """N > 256 takes the thread-per-env kernel: bit-exact with the reference op order."""
    g = golden("gae_ref")
    r1, v1, d1, l1 = g["c0_r"], g["c0_v"], g["c0_d"], g["c0_last"]
    T, N = r1.shape[0], 1024
    rs = np.random.RandomState(1)
    r = np.repeat(r1[:, None], N, 1) + rs.randn(T, N).astype(np.float32) * 0.01
    v = np.repeat(v1[:, None], N, 1) + rs.randn(T, N).astype(np.float32) * 0.1
    d = (rs.rand(T, N) < 0.01).astype(np.float32)
    d[:, 0] = d1
    r[:, 0], v[:, 0] = r1, v1
    lv = rs.randn(N).astype(np.float32)
    lv[0] = l1
    adv, ret = _gae(device, r, v, d, lv)
    assert (adv[:, 0] == g["c0_adv"]).all() and (ret[:, 0] == g["c0_ret"]).all()
    oadv, oret = oracle.gae_tn(r, v, d, lv)
    assert (adv == oadv).all() and (ret == oret).all()


@pytest.mark.parametrize("N", [1, 7, 256, 257, 4096])
def test_gae_and_normalisation_shapes(oracle, device, N):
    from merlin import _native as nat

    T = 256
    rs = np.random.RandomState(N)
    r = ((rs.rand(T, N) < 0.05) * rs.rand(T, N)).astype(np.float32)
    v = rs.randn(T, N).astype(np.float32)
    d = (rs.rand(T, N) < 0.02).astype(np.float32)
    lv = rs.randn(N).astype(np.float32)
    stats = torch.zeros(3, dtype=torch.float64, device=device)
    adv, ret = _gae(device, r, v, d, lv, stats=stats)
    oadv, oret = oracle.gae_tn(r, v, d, lv)
    np.testing.assert_allclose(adv, oadv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ret, oret, rtol=1e-5, atol=1e-5)
    s = stats.cpu().numpy()
    assert s[0] == T * N
    # the moments are the f64 sums of the kernel's own f32 advantages
    np.testing.assert_allclose(s[1], adv.astype(np.float64).sum(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(s[2], (adv.astype(np.float64) ** 2).sum(), rtol=1e-12)
    a = torch.from_numpy(adv).to(device)
    norm = nat.adv_normalize(a, stats).cpu().numpy()
    np.testing.assert_allclose(norm, oracle.adv_normalize(oadv), rtol=1e-5, atol=1e-5)
    # property at full size: normalised advantages have mean 0, unbiased std 1
    assert abs(norm.astype(np.float64).mean()) < 1e-5
    assert abs(norm.astype(np.float64).std(ddof=1) - 1.0) < 1e-4


def test_adv_normalisation_vs_reference(golden, device):
    from merlin import _native as nat

    g = golden("gae_ref")
    for k in range(int(g["ncases"])):
        stats = torch.zeros(3, dtype=torch.float64, device=device)
        _gae(device, g[f"c{k}_r"], g[f"c{k}_v"], g[f"c{k}_d"], g[f"c{k}_last"], stats=stats)
        a = torch.from_numpy(g[f"c{k}_adv"]).to(device)
        norm = nat.adv_normalize(a, stats).cpu().numpy()
        np.testing.assert_allclose(norm, g[f"c{k}_advnorm"], rtol=1e-5, atol=1e-5)


def _gae_case(T, N, seed):
    """Rewards / values / bootstrap of tests/test_gpu_obs_gae.py's shape test, and the done patterns that put an
    episode end on every seam of the two kernels: the wave kernel cuts T into 64 chunks of L = ceil(T / 64) steps
    (lane k owns t = kL .. kL + L - 1), the thread kernel walks t = T - 2 .. 0 in load batches of 8 and a tail."""
    rs = np.random.RandomState(seed)
    r = ((rs.rand(T, N) < 0.05) * rs.rand(T, N)).astype(np.float32)
    v = rs.randn(T, N).astype(np.float32)
    lv = rs.randn(N).astype(np.float32)
    L = -(-T // 64)
    z = np.zeros((T, N), dtype=np.float32)
    pats = {"none": z, "all": z + 1, "last": z.copy(), "first": z.copy(), "chunk_edges": z.copy(),
            "batch_edges": z.copy(), "random": (rs.rand(T, N) < 0.02).astype(np.float32)}
    pats["last"][T - 1] = 1
    pats["first"][0] = 1
    pats["chunk_edges"][::L] = 1          # t = kL: the first step of every chunk
    pats["chunk_edges"][L - 1::L] = 1     # t = kL - 1: the last step of the chunk before
    for t in range(T - 1):                # the first and the last step of every load batch of the thread kernel
        if (T - 2 - t) % 8 in (0, 7):
            pats["batch_edges"][t] = 1
    return r, v, lv, pats


def _gae_prefilled(device, r, v, d, lv, gamma):
    """nat.gae into adv / ret prefilled with NaN, with stats: (adv, ret, stats) on the host."""
    from merlin import _native as nat

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)  # noqa: E731
    adv = torch.full(r.shape, float("nan"), dtype=torch.float32, device=device)
    ret = torch.full(r.shape, float("nan"), dtype=torch.float32, device=device)
    stats = torch.full((3,), float("nan"), dtype=torch.float64, device=device)
    nat.gae(t(r), t(v), t(d), t(lv), gamma, 0.95, adv=adv, ret=ret, stats=stats)
    return adv.cpu().numpy(), ret.cpu().numpy(), stats.cpu().numpy()


def _check_gae_stats(s, adv, T, N):
    # as test_gae_and_normalisation_shapes: the count exact, the moments the f64 sums of the kernel's own advantages
    assert s[0] == T * N
    np.testing.assert_allclose(s[1], adv.astype(np.float64).sum(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(s[2], (adv.astype(np.float64) ** 2).sum(), rtol=1e-12)


@pytest.mark.parametrize("T", [1, 2, 8, 9, 10, 16, 17, 31])
@pytest.mark.parametrize("N", [257, 300])
def test_gae_thread_kernel_ragged_T(oracle, device, N, T):
    """N > 256, the thread-per-env kernel: the step T - 1 alone (T = 1), no load batch (T - 1 < 8), exactly one
    (T = 9), one and a tail (10, 16), two and no tail (17), three and a tail (31); a second block with 1 / 44 live
    threads.  Bit-exact with the reference's op order, every element written."""
    r, v, lv, pats = _gae_case(T, N, 100 * N + T)
    for name, d in pats.items():
        adv, ret, s = _gae_prefilled(device, r, v, d, lv, 0.99)
        assert np.isfinite(adv).all() and np.isfinite(ret).all(), name
        oadv, oret = oracle.gae_tn(r, v, d, lv)
        assert (adv == oadv).all() and (ret == oret).all(), name
        _check_gae_stats(s, adv, T, N)


@pytest.mark.parametrize("T", [1, 2, 5, 63, 64, 65, 100, 127, 129, 300])
@pytest.mark.parametrize("N", [1, 3, 256])
def test_gae_wave_kernel_ragged_T(oracle, device, N, T):
    """N <= 256, one wave per env, the horizons merlin/evaluation.py and merlin/fomaml.py pass: T < 64 leaves lanes
    empty (L = 1), T = 65 .. 127 gives chunks of 2 with the last lanes empty and one part-filled (65, 127), 129 and
    300 chunks of 3 and 5.  Against the oracle at this file's 1e-5, both gammas, every element written."""
    r, v, lv, pats = _gae_case(T, N, 100 * N + T)
    for gamma in (0.99, 0.995):
        for name, d in pats.items():
            adv, ret, s = _gae_prefilled(device, r, v, d, lv, gamma)
            assert np.isfinite(adv).all() and np.isfinite(ret).all(), (name, gamma)
            oadv, oret = oracle.gae_tn(r, v, d, lv, gamma=gamma)
            np.testing.assert_allclose(adv, oadv, rtol=1e-5, atol=1e-5, err_msg=f"{name} {gamma}")
            np.testing.assert_allclose(ret, oret, rtol=1e-5, atol=1e-5, err_msg=f"{name} {gamma}")
            _check_gae_stats(s, adv, T, N)


@pytest.mark.parametrize("n", [2 ** 20 + 1, 3 * 2 ** 20 + 5])
def test_adv_normalisation_beyond_the_grid_cap(oracle, device, n):
    """More than 4,096 blocks of 256 elements: the grid-stride loop takes a second (2^20 + 1: for one thread only)
    and a fourth turn.  stats are the host's float64 sums."""
    from merlin import _native as nat

    a = np.random.RandomState(n % 1000).randn(n).astype(np.float32)
    a64 = a.astype(np.float64)
    stats = torch.tensor([float(n), a64.sum(), (a64 * a64).sum()], dtype=torch.float64, device=device)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    nat.adv_normalize(torch.from_numpy(a).to(device), stats, out=out)
    np.testing.assert_allclose(out.cpu().numpy(), oracle.adv_normalize(a), rtol=1e-5, atol=1e-5)


def test_adv_normalisation_of_a_constant_is_exact_zero(device):
    """A constant c: the exact sums give a variance of exactly 0; a sum of squares one unit in the last place low
    (what a rounded summation can return) gives a slightly negative one, which the kernel clamps.  Both normalise
    to exact zeros -- (c - c) / 1e-8 -- where an unclamped square root would give NaN."""
    from merlin import _native as nat

    n = 2 ** 20 + 1
    c = np.float32(0.3)
    s1, s2 = float(n) * float(c), float(n) * (float(c) * float(c))  # n c exact (46 bits), n c^2 rounded once
    a = torch.full((n,), float(c), dtype=torch.float32, device=device)
    for sq in (s2, float(np.nextafter(s2, 0.0))):
        mean = s1 / n
        var = (sq - s1 * mean) / (n - 1.0)  # k_adv_normalize's float64 expression
        assert mean == float(c) and (var < 0.0 if sq != s2 else var == 0.0)
        stats = torch.tensor([float(n), s1, sq], dtype=torch.float64, device=device)
        out = nat.adv_normalize(a, stats)
        assert (out == 0).all()
