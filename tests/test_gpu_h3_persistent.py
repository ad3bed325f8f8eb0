"""GPU: the persistent forms of fc1's plane-operand NT GEMMs (csrc/merlin_h3p.hip k_h3_pq / k_h3_pqg with PERS: one
block per CU walking a static list of tiles, the DMA ring and the C stores carried across tile boundaries).

The walk changes when things happen, never what is summed: every output must carry the bits of the one-tile-per-block
kernel (cfg 77 against 78 for the input gradient, 75 against 76 for the forward over gathered rows, with the bias +
ReLU epilogue alone and with the heads), call after call.  The walk itself is reached through the block-count override
(_native.h3_walk_blocks), so that its cases do not depend on the device's CU count:

    M = 1, default grid        one tile per tower: most blocks get nothing
    M = 777, 7 blocks          7 row tiles, ragged last one; 6 tiles per block in the input gradient (K = 512: 16 k
                               steps, so the ring's stage turns by one per tile -- all three turns and the wrap)
    M = 777, 5 blocks          uneven tile counts per block
    M = 20011, default grid    3-4 tiles per block, both towers in one block's list
    M = 20011, scale 1e-7      the gradient's magnitudes (only the per-tensor exponent keeps them in f16 range)

One case per kernel is also held to float64 with test_gpu_h3.py's tolerance (torch's own fp32 GEMM error on the same
operands, floor 2^-21), and 20 calls of the multi-tile cases are compared with the first."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -21  # test_gpu_h3.py: one product's own error bound
CASES = [(1, 1.0, None), (777, 1.0, 7), (777, 1.0, 5), (20011, 1.0, None), (20011, 1e-7, None)]
DGRAD_TILE, DGRAD_WALK, FWD_TILE, FWD_WALK = 77, 78, 75, 76


def _err(C, C64, den):
    return float(((C.double() - C64).abs() / den.clamp_min(1e-300)).max())


def _walk(blocks):
    from merlin import _native as nat

    return nat.h3_walk_blocks(blocks or 0)


_CACHE = {}


def _dgrad(device, M, scale):
    """The input gradient's operands as planes (N = 576, K = 512) and the one-tile kernel's result."""
    from merlin import _native as nat

    key = ("dgrad", M, scale)
    if key not in _CACHE:
        g = torch.Generator(device=device).manual_seed(5 * M + 1)
        A = torch.randn(2, M, 512, device=device, generator=g) * scale
        B = torch.randn(2, 576, 512, device=device, generator=g) / 512 ** 0.5
        amA, amB = nat.h3_amax(A), nat.h3_amax(B)
        Ap, Bp = nat.h3_split(A, amA), nat.h3_split(B, amB)
        ref = nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, cfg=DGRAD_TILE)
        _CACHE[key] = (A, B, Ap, amA, Bp, amB, ref)
    return _CACHE[key]


def _fwd(device, M, scale):
    """The forward's operands (N = 512, K = 576): a3 as planes read through a random row map with repeats, the head
    weights, and the one-tile kernel's results for both epilogues."""
    from merlin import _native as nat

    key = ("fwd", M, scale)
    if key not in _CACHE:
        g = torch.Generator(device=device).manual_seed(3 * M + 2)
        A = torch.relu(torch.randn(2, M, 576, device=device, generator=g)) * scale
        B = torch.randn(2, 512, 576, device=device, generator=g) / 576 ** 0.5
        nc = M * 9
        rows = torch.randint(0, max(nc // 2, 1), (nc,), device=device, generator=g, dtype=torch.int32)  # repeats
        bias = torch.randn(2, 512, device=device, generator=g) * scale
        Wa = torch.randn(3, 512, device=device, generator=g) / 512 ** 0.5
        Wc = torch.randn(1, 512, device=device, generator=g) / 512 ** 0.5
        amA, amB = nat.h3_amax(A), nat.h3_amax(B)
        Ap, Bp = nat.h3_split(A, amA), nat.h3_split(B, amB)
        h1 = nat.h3_gemm_nt_heads(Ap, amA, Bp, amB, bias, Wa, Wc, cfg=FWD_TILE, rows=rows, heads=False)
        h2, part = _heads(Ap, amA, Bp, amB, bias, Wa, Wc, rows, FWD_TILE)
        _CACHE[key] = (A, B, Ap, amA, Bp, amB, rows, bias, Wa, Wc, h1, h2, part)
    return _CACHE[key]


def _heads(Ap, amA, Bp, amB, bias, Wa, Wc, rows, cfg):
    """(h, (logits, value, partials)) of the forward with the heads' epilogue: the partials read back as the kernel
    wrote them, through the binding's own call."""
    from merlin import _native as nat

    M = int(Ap.shape[1])
    P = int(nat.lib().merlin_h3_heads_parts(512, cfg))
    assert P == 8
    out = torch.empty((2, M, 512), dtype=torch.float32, device=Ap.device)
    part = torch.full((2, P, M, 4), float("nan"), dtype=torch.float32, device=Ap.device)
    nat.check(nat.lib().merlin_h3_gemm_nt_heads_planes(
        nat.ptr(Ap), nat.ptr(amA), nat.ptr(Bp), nat.ptr(amB), M, 512, 576, M * 576, 512 * 576, nat.ptr(bias),
        nat.ptr(out), M * 512, nat.ptr(rows), nat.ptr(Wa), 3, nat.ptr(Wc), nat.ptr(part), cfg,
        nat.stream_of(Ap)), "merlin_h3_gemm_nt_heads_planes")
    h, logits, value = nat.h3_gemm_nt_heads(Ap, amA, Bp, amB, bias, Wa, Wc, cfg=cfg, rows=rows)
    assert torch.equal(h, out)
    return out, (logits, value, part)


def _same_heads(a, b):
    # the partials' lanes of actions the tower does not have are written too (zero weights): all of them compared
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("M,scale,blocks", CASES)
def test_dgrad_walk_bitwise(device, M, scale, blocks):
    from merlin import _native as nat

    _, _, Ap, amA, Bp, amB, ref = _dgrad(device, M, scale)
    with _walk(blocks):
        got = nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, cfg=DGRAD_WALK)
        again = nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, cfg=DGRAD_WALK)
    assert torch.equal(got, ref)
    assert torch.equal(again, ref)
    bias = torch.randn(2, 576, device=device)  # the bias + ReLU epilogue (its constants change with the column tile)
    with _walk(blocks):
        gb = nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, bias=bias, cfg=DGRAD_WALK)
    assert torch.equal(gb, nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, bias=bias, cfg=DGRAD_TILE))


@pytest.mark.parametrize("M,scale,blocks", CASES)
def test_fwd_walk_bitwise(device, M, scale, blocks):
    from merlin import _native as nat

    _, _, Ap, amA, Bp, amB, rows, bias, Wa, Wc, h1, h2, part = _fwd(device, M, scale)
    assert torch.equal(h1, h2)  # the heads' epilogue leaves h as the plain one
    with _walk(blocks):
        g1 = nat.h3_gemm_nt_heads(Ap, amA, Bp, amB, bias, Wa, Wc, cfg=FWD_WALK, rows=rows, heads=False)
        g2, gp = _heads(Ap, amA, Bp, amB, bias, Wa, Wc, rows, FWD_WALK)
        a1 = nat.h3_gemm_nt_heads(Ap, amA, Bp, amB, bias, Wa, Wc, cfg=FWD_WALK, rows=rows, heads=False)
        a2, ap = _heads(Ap, amA, Bp, amB, bias, Wa, Wc, rows, FWD_WALK)
    assert torch.equal(g1, h1) and torch.equal(a1, h1)
    assert torch.equal(g2, h2) and torch.equal(a2, h2)
    assert _same_heads(gp, part) and _same_heads(ap, part)


def test_default_cfgs_bitwise(device):
    """cfg 62 / 60, the update's, whichever form they select: the one-tile kernels' bits."""
    from merlin import _native as nat

    _, _, Ap, amA, Bp, amB, ref = _dgrad(device, 777, 1.0)
    assert torch.equal(nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, cfg=62), ref)
    _, _, Ap, amA, Bp, amB, rows, bias, Wa, Wc, h1, h2, part = _fwd(device, 777, 1.0)
    g2, gp = _heads(Ap, amA, Bp, amB, bias, Wa, Wc, rows, 60)
    assert torch.equal(g2, h2) and _same_heads(gp, part)


@pytest.mark.parametrize("M,scale,blocks", [(777, 1.0, 7), (20011, 1e-7, None)])
def test_walk_vs_float64(device, M, scale, blocks):
    """test_gemm_nt_planes_vs_float64's bound on the persistent kernels: the error against a float64 product of the
    same fp32 operands, over sum_k |a_k b_k|, no larger than torch's own fp32 GEMM's (floor: one product's bound).
    The forward with a zero bias: its ReLU only shrinks a difference."""
    from merlin import _native as nat

    A, B, Ap, amA, Bp, amB, _ = _dgrad(device, M, scale)
    C64 = torch.bmm(A.double(), B.double().transpose(1, 2))
    den = torch.bmm(A.abs().double(), B.abs().double().transpose(1, 2))
    tol = max(_err(torch.bmm(A, B.transpose(1, 2)), C64, den), FLOOR)
    with _walk(blocks):
        C = nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, cfg=DGRAD_WALK)
    e = _err(C, C64, den)
    print(f"dgrad walk M={M} scale={scale}: err {e:.3e} tol {tol:.3e}")
    assert e <= tol

    A, B, Ap, amA, Bp, amB, rows, _, Wa, Wc, *_ = _fwd(device, M, scale)
    Ae = A.view(2, M * 9, 64)[:, rows.long()].reshape(2, M, 576)
    C64 = torch.bmm(Ae.double(), B.double().transpose(1, 2))
    den = torch.bmm(Ae.abs().double(), B.abs().double().transpose(1, 2))
    tol = max(_err(torch.relu(torch.bmm(Ae, B.transpose(1, 2))), torch.relu(C64), den), FLOOR)
    zero = torch.zeros(2, 512, device=device)
    with _walk(blocks):
        h = nat.h3_gemm_nt_heads(Ap, amA, Bp, amB, zero, Wa, Wc, cfg=FWD_WALK, rows=rows, heads=False)
    e = _err(h, torch.relu(C64), den)
    print(f"fwd walk M={M} scale={scale}: err {e:.3e} tol {tol:.3e}")
    assert e <= tol


def test_walk_repeats(device):
    """A new synchronisation structure: 20 calls each of the multi-tile cases, every output compared with the first
    (which the tests above hold to the one-tile kernels' bits)."""
    from merlin import _native as nat

    for M, blocks in ((777, 7), (20011, None)):
        _, _, Ap, amA, Bp, amB, ref = _dgrad(device, M, 1.0)
        _, _, Fp, fmA, Gp, fmB, rows, bias, Wa, Wc, h1, h2, part = _fwd(device, M, 1.0)
        with _walk(blocks):
            d = [nat.h3_gemm_nt_planes(Ap, amA, Bp, amB, cfg=DGRAD_WALK) for _ in range(20)]
            f = [_heads(Fp, fmA, Gp, fmB, bias, Wa, Wc, rows, FWD_WALK) for _ in range(20)]
        assert torch.equal(d[0], ref) and torch.equal(f[0][0], h2) and _same_heads(f[0][1], part)
        assert all(torch.equal(x, d[0]) for x in d[1:])
        assert all(torch.equal(h, f[0][0]) and _same_heads(p, f[0][1]) for h, p in f[1:])


def test_walk_blocks_argument(device):
    from merlin import _native as nat

    with pytest.raises(nat.MerlinNativeError):
        with nat.h3_walk_blocks(-1):
            pass
