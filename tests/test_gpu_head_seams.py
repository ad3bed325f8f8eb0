"""GPU: the tower epilogues (csrc/merlin_head.hip) at the edges of their partitions, on inputs of small integers.

Every sum of such a case is exact in fp32 in any order (tests/fold_ref.py: every sum of |terms| < 2^24, asserted by the
builders), so each output must equal the float64 reference BIT FOR BIT -- no tolerance: a dropped, doubled or
misrouted row moves a sum by at least 1 (the builders also assert that every row reaches an output).  Every call is
made twice and must return the same bits.  The seams:

  k_relu_bwd_colsum, k_colsum   32 rows per block up to EPI_MAX_BLOCKS = 512 blocks (rows 1 .. 257: 1, 2, 3, 7, 8, 9
                                blocks); above 16384 rows per = ceil(rows / 512) = 33 rows and the trailing blocks
                                are empty (16385, 16897); 16896 = 512 x 33 fills them all.  R = 256 / (cols / 4) rows
                                in flight: cols 4, 64, 512, 1024 -> R = 256, 16, 2, 1
  k_fold_cols, k_head_fold      32 outputs per block, 8 slices over the blocks' partials (nblk 1, 2, 3, 7, 8, 9, 512);
                                T x cols = 4 and (1 + A) H + 2 H = 20 outputs: less than one block (the k < total guard)
  k_head_bwd<NA>                the same blocks; 4 rows per thread per round with clamped reads (H = 512: 8 rows per
                                round, n = 1, 7, 8, 9; H = 64: 64 rows, n = 63, 64, 65, 129; H = 1024: R = 1; H = 4);
                                above the cap per = 33, 39, 40, 41 (per mod 8 = 1, 7, 0, 1); NA = 3 for A <= 3, else 8
  k_heads_fwd<NA>               16 rows per block round, 2048 blocks: n = 15, 16, 17, 32767, 32768, 32769, 65537
  k_bias_relu                   4096 blocks x 256 float4: 2^20 float4 per grid stride

and one float case per summing kernel: its error against float64, relative to the sum of |terms|, no larger than
twice torch's own fp32 error on the same operands (floor 2^-23, the convention of tests/test_gpu_window_bwd.py)."""
import pytest
import torch

import fold_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
ROWS = (1, 31, 32, 33, 64, 65, 224, 256, 257, 16383, 16384, 16385, 16896, 16897)
COLS = (4, 64, 512, 1024)


def _eq(got, ref):
    return bool(torch.equal(got.double(), ref))


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("rows", ROWS)
def test_relu_bwd_exact(device, rows, T):
    from merlin import _native as nat

    for cols in COLS:
        y, dy = R.relu_case(T, rows, cols, rows + cols, device)
        rdz, rdb = R.relu_bwd(y, dy)
        dz, db = nat.relu_bwd(y, dy)
        assert _eq(dz, rdz) and _eq(db, rdb), (cols, float((db.double() - rdb).abs().max()))
        dz2, db2 = nat.relu_bwd(y, dy)
        assert torch.equal(dz, dz2) and torch.equal(db, db2)
        g = dy.clone()  # in place: dz written over dy
        dz3, db3 = nat.relu_bwd(y, g, out=g)
        assert dz3 is g and torch.equal(g, dz) and torch.equal(db3, db), cols


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("rows", ROWS)
def test_colsum_exact(device, rows, T):
    from merlin import _native as nat

    for cols in COLS:
        x = R.colsum_case(T, rows, cols, rows + cols + 1, device)
        ref = R.colsum(x)
        out = nat.colsum(x)
        assert _eq(out, ref), (cols, float((out.double() - ref).abs().max()))
        assert torch.equal(out, nat.colsum(x))
    x = R.colsum_case(T, rows, 64, rows + 2, device, taps=9)  # tap 0 of dQ [T, rows, 9, 64]: strided rows
    assert x.stride() == (rows * 576, 576, 1)
    out = nat.colsum(x)
    assert _eq(out, R.colsum(x)) and torch.equal(out, nat.colsum(x))


@pytest.mark.parametrize("T,rows,cols", [(1, 2 ** 20 - 1, 4), (1, 2 ** 20, 4), (1, 2 ** 20 + 1, 4), (2, 4097, 64)])
def test_bias_relu_exact(device, T, rows, cols):
    """relu(z + b) in place with NaN, +-inf and -0.0 among the inputs: NaN stays, the rest is max(z + b, 0) by value
    (fold_ref's module docstring); the grid-stride seam, and a tower boundary inside a block."""
    from merlin import _native as nat

    z, b = R.bias_relu_case(T, rows, cols, rows, device)
    ref = R.bias_relu(z, b)
    assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any())
    out = nat.bias_relu_(z.clone(), b)
    assert R.same(out, ref)
    out2 = nat.bias_relu_(z.clone(), b)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))


HEAD_CASES = [(n, 512, 3) for n in (1, 7, 8, 9, 33, 62, 64, 65, 257, 16384, 16385, 19968, 20480, 20992)] \
    + [(n, 512, A) for n in (65, 16385) for A in (1, 2, 4, 8)] \
    + [(n, 64, 3) for n in (63, 64, 65, 129)] + [(33, 1024, 3), (33, 4, 2)]


@pytest.mark.parametrize("n,H,A", HEAD_CASES)
def test_head_bwd_exact(device, n, H, A):
    from merlin import _native as nat

    h, dl, dv, wa, wc = R.head_case(n, H, A, n + H + A, device)
    rdz, rdb, rdwa, rdwc = R.head_bwd(h, dl, dv, wa, wc)
    got = []
    for _ in range(2):
        amax = torch.zeros(2, dtype=torch.int32, device=device)
        dz, db4, dwa, dwc = nat.head_bwd(h, dl, dv, wa, wc, amax=amax)
        got.append((dz, db4, dwa, dwc, amax))
    dz, db4, dwa, dwc, amax = got[0]
    assert _eq(dz, rdz)
    assert _eq(db4, rdb), float((db4.double() - rdb).abs().max())
    assert _eq(dwa, rdwa), float((dwa.double() - rdwa).abs().max())
    assert _eq(dwc, rdwc), float((dwc.double() - rdwc).abs().max())
    assert torch.equal(amax, rdz.abs().amax((1, 2)).float().view(torch.int32))  # max |dz[t]| as float bits
    assert all(torch.equal(a, b) for a, b in zip(got[0], got[1]))
    # without amax: the same outputs
    assert all(torch.equal(a, b) for a, b in zip(got[0][:4], nat.head_bwd(h, dl, dv, wa, wc)))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 32767, 32768, 32769, 65537])
def test_heads_fwd_exact(device, n):
    from merlin import _native as nat

    for A in (1, 3, 4, 8):
        for bias in (False, True):
            h, wa, wc, ba, bc = R.heads_fwd_case(n, A, bias, n + A, device)
            rl, rv = R.heads_fwd(h, wa, wc, ba, bc)
            logits, value = nat.heads_fwd(h, wa, wc, ba, bc)
            assert _eq(logits, rl) and _eq(value, rv), (A, bias)
            l2, v2 = nat.heads_fwd(h, wa, wc, ba, bc)
            assert torch.equal(logits, l2) and torch.equal(value, v2)


# ----------------------------------------------------------------------------------------------------------------------
# One float case per summing kernel: error relative to the sum of |terms|, beside torch's own fp32 error.
def _rel(x, x64, den):
    return float(((x.double() - x64).abs() / den.clamp_min(1e-300)).max())


def _held(name, got, torch32, ref64, den):
    e, e0 = _rel(got, ref64, den), _rel(torch32, ref64, den)
    print("%s: kernel %.3g, torch fp32 %.3g (x 2^-24: %.2f, %.2f)" % (name, e, e0, e * 2 ** 24, e0 * 2 ** 24))
    assert e <= max(2.0 * e0, FLOOR), (name, e, e0)


def test_relu_bwd_and_colsum_float(device):
    from merlin import _native as nat

    g = torch.Generator(device=device)
    g.manual_seed(41)
    y = torch.randn(2, 16897, 512, device=device, generator=g)
    dy = torch.randn(2, 16897, 512, device=device, generator=g)
    dz32 = torch.where(y > 0, dy, torch.zeros_like(dy))
    dz, db = nat.relu_bwd(y, dy)
    assert torch.equal(dz, dz32)
    _held("relu_bwd dbias", db, dz32.sum(1), dz32.double().sum(1), dz32.double().abs().sum(1))
    _held("colsum", nat.colsum(dy), dy.sum(1), dy.double().sum(1), dy.double().abs().sum(1))


def test_head_bwd_float(device):
    from merlin import _native as nat

    g = torch.Generator(device=device)
    g.manual_seed(42)
    n, H, A = 16385, 512, 3
    h = torch.relu(torch.randn(2, n, H, device=device, generator=g))
    dl, dv = torch.randn(n, A, device=device, generator=g), torch.randn(n, device=device, generator=g)
    wa, wc = torch.randn(A, H, device=device, generator=g), torch.randn(H, device=device, generator=g)
    dz, db4, dwa, dwc = nat.head_bwd(h, dl, dv, wa, wc)
    rdz, rdb, rdwa, rdwc = R.head_bwd(h, dl, dv, wa, wc)
    zero = torch.zeros((), device=device)
    t_dz = torch.where(h > 0, torch.stack([dl @ wa, dv[:, None] * wc[None]]), zero)
    den_dz = torch.stack([dl.double().abs() @ wa.double().abs(), dv.double().abs()[:, None] * wc.double().abs()[None]])
    _held("head_bwd dz", dz, t_dz, rdz, den_dz)
    # the bias gradient sums the fp32 dz rows: its terms are the kernel's own dz (checked above)
    _held("head_bwd db4", db4, dz.sum(1), dz.double().sum(1), dz.double().abs().sum(1))
    _held("head_bwd dWa", dwa, dl.t() @ h[0], rdwa, dl.double().abs().t() @ h.double()[0].abs())
    _held("head_bwd dwc", dwc, dv @ h[1], rdwc, dv.double().abs() @ h.double()[1].abs())


def test_heads_fwd_float(device):
    from merlin import _native as nat

    g = torch.Generator(device=device)
    g.manual_seed(43)
    n, A = 32769, 3
    h = torch.relu(torch.randn(2, n, 512, device=device, generator=g))
    wa = torch.randn(A, 512, device=device, generator=g) / 512 ** 0.5
    wc = torch.randn(512, device=device, generator=g) / 512 ** 0.5
    logits, value = nat.heads_fwd(h, wa, wc)
    rl, rv = R.heads_fwd(h, wa, wc)
    _held("heads_fwd logits", logits, h[0] @ wa.t(), rl, h.double()[0].abs() @ wa.double().abs().t())
    _held("heads_fwd value", value, h[1] @ wc, rv, h.double()[1].abs() @ wc.double().abs())
