"""GPU: merlin_group_clip_sgd (csrc/merlin_fewshot.hip, nat.group_clip_sgd) -- clip_grad_norm_(0.5) + SGD for G
independent parameter sets -- against a float64 restatement per task and against the torch chain it replaces
(FOMAML._clip_per_task + fast - lr * g).

G = 4, tensors of 1, 3, 1023, 1025 and 4097 elements per task (around the 1024-element block).  Task 0: gradient
norm below 0.5 (coefficient 1); task 1: norm about 50; task 2: all-zero gradients; task 3: one NaN element.
The kernel takes lr as a float, so the restatement uses float32(lr)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G, LR, MAX_NORM = 4, 0.01, 0.5
SHAPES = [(1,), (3,), (1023,), (5, 205), (17, 241)]
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(5)
    params = [rs.randn(G, *s).astype(np.float32) for s in SHAPES]
    grads = [rs.randn(G, *s).astype(np.float32) for s in SHAPES]
    n_all = sum(int(np.prod(s)) for s in SHAPES)
    for g in grads:
        g[0] *= np.float32(0.3 / np.sqrt(n_all))  # norm ~0.3
        g[1] *= np.float32(50.0 / np.sqrt(n_all))  # norm ~50
        g[2] = 0.0
    clean = [g.copy() for g in grads]
    grads[2][3, 1000] = np.nan
    return params, grads, clean


def _run(device, params, grads):
    from merlin import _native as nat

    p = [torch.from_numpy(x.copy()).to(device) for x in params]
    g = [torch.from_numpy(x.copy()).to(device) for x in grads]
    norm = nat.group_clip_sgd(p, g, LR, MAX_NORM)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in p], [x.cpu().numpy() for x in g], norm.cpu().numpy()


def _restate(params, grads, task):
    """(norm, clipped gradients, new parameters) of one task in float64."""
    norm = np.sqrt(sum((g[task].astype(np.float64) ** 2).sum() for g in grads))
    coef = min(MAX_NORM / (norm + 1e-6), 1.0)
    gc = [g[task].astype(np.float64) * coef for g in grads]
    lr = float(np.float32(LR))
    return norm, gc, [p[task].astype(np.float64) - lr * c for p, c in zip(params, gc)]


def test_matches_float64_restatement_per_task(device, case):
    params, grads, _ = case
    p1, g1, norm = _run(device, params, grads)
    norms = [_restate(params, grads, t)[0] for t in range(3)]
    print("norms", norm, norms)
    assert norms[0] < MAX_NORM and 40 < norms[1] < 60 and norms[2] == 0.0
    for t in range(3):
        ref_norm, ref_g, ref_p = _restate(params, grads, t)
        assert abs(norm[t] - ref_norm) <= 1e-6 * ref_norm, (t, norm[t], ref_norm)
        for i in range(len(SHAPES)):
            eg = np.abs(g1[i][t] - ref_g[i])
            ep = np.abs(p1[i][t] - ref_p[i])
            bound_p = 4 * EPS * (np.abs(params[i][t]) + LR * np.abs(grads[i][t]))
            print(f"task {t} tensor {i}: grad err/bound {np.max(eg / np.maximum(4 * EPS * np.abs(ref_g[i]), 1e-300)):.3f}"
                  f" param err/bound {np.max(ep / bound_p):.3f}")
            assert (eg <= 4 * EPS * np.abs(ref_g[i])).all(), (t, i)
            assert (ep <= bound_p).all(), (t, i)
    for i in range(len(SHAPES)):  # zero gradients: the parameters keep their bits
        assert (p1[i][2].view(np.int32) == params[i][2].view(np.int32)).all(), i
        assert (g1[i][2] == 0).all()


def test_nan_stays_inside_its_task(device, case):
    params, grads, clean = case
    p1, g1, norm = _run(device, params, grads)
    p2, g2, norm2 = _run(device, params, clean)
    assert np.isnan(norm[3]) and np.isfinite(norm2).all()
    for i in range(len(SHAPES)):
        assert np.isnan(p1[i][3]).all() and np.isnan(g1[i][3]).all(), i
        assert np.isfinite(p2[i]).all()
        assert (p1[i][:3].view(np.int32) == p2[i][:3].view(np.int32)).all(), i
        assert (g1[i][:3].view(np.int32) == g2[i][:3].view(np.int32)).all(), i
    assert (norm[:3].view(np.int32) == norm2[:3].view(np.int32)).all()


def test_bitwise_reproducible(device, case):
    params, grads, _ = case
    a, b = _run(device, params, grads), _run(device, params, grads)
    for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
        assert (x.view(np.int32) == y.view(np.int32)).all()


def test_matches_the_torch_chain(device, case):
    """FOMAML._clip_per_task + fast - lr * g (fp32 sums of squares): the parameters agree to the restatement's
    bound; the NaN task is NaN on both."""
    from merlin.fomaml import FOMAML

    params, grads, _ = case
    p1, _, norm = _run(device, params, grads)
    names = [str(i) for i in range(len(SHAPES))]
    gd = {n: torch.from_numpy(g.copy()).to(device) for n, g in zip(names, grads)}
    clipped, tnorm = FOMAML._clip_per_task(gd, MAX_NORM)
    for i, n in enumerate(names):
        ref = (torch.from_numpy(params[i]).to(device) - LR * clipped[n]).cpu().numpy()
        assert np.isnan(ref[3]).all() and np.isnan(p1[i][3]).all()
        err = np.abs(p1[i][:3].astype(np.float64) - ref[:3].astype(np.float64))
        bound = 4 * EPS * (np.abs(params[i][:3]) + LR * np.abs(grads[i][:3]))
        print(f"tensor {i}: err/bound {np.max(err / bound):.3f}")
        assert (err <= bound).all(), i
    assert np.allclose(norm[:3], tnorm.cpu().numpy()[:3], rtol=1e-5)


def test_argument_checks(device):
    from merlin import _native as nat

    p = torch.zeros(2, 8, device=device)
    assert nat.group_clip_sgd([], [], LR, MAX_NORM) is None  # no tensors: nothing to do
    with pytest.raises(ValueError):
        nat.group_clip_sgd([p], [p[:, :4].contiguous()], LR, MAX_NORM)
    with pytest.raises(nat.MerlinNativeError):
        nat.group_clip_sgd([p], [p.double()], LR, MAX_NORM)
    assert nat.group_clip_sgd([p[:0]], [p[:0]], LR, MAX_NORM).numel() == 0  # G = 0


EDGE_NUMEL = [1, 1023, 1024, 1025, 2049, 4096]  # around the 1,024-element chunk


def _edge_case(G_, shapes, seed):
    """Task 0 (and 2): gradient norm about 50, clipped; task 1: about 0.3, coefficient 1."""
    rs = np.random.RandomState(seed)
    params = [rs.randn(G_, *s).astype(np.float32) for s in shapes]
    grads = [rs.randn(G_, *s).astype(np.float32) for s in shapes]
    n_all = sum(int(np.prod(s)) for s in shapes)
    for g in grads:
        g[0::2] *= np.float32(50.0 / np.sqrt(n_all))
        g[1::2] *= np.float32(0.3 / np.sqrt(n_all))
    return params, grads


def _check_restatement(params, grads, p1, g1, norm, G_):
    for t in range(G_):
        ref_norm, ref_g, ref_p = _restate(params, grads, t)
        assert (40 < ref_norm < 60) if t % 2 == 0 else ref_norm < MAX_NORM
        assert abs(norm[t] - ref_norm) <= 1e-6 * ref_norm, (t, norm[t], ref_norm)
        for i in range(len(params)):
            eg = np.abs(g1[i][t] - ref_g[i])
            ep = np.abs(p1[i][t] - ref_p[i])
            assert (eg <= 4 * EPS * np.abs(ref_g[i])).all(), (t, i)
            assert (ep <= 4 * EPS * (np.abs(params[i][t]) + LR * np.abs(grads[i][t]))).all(), (t, i)


@pytest.mark.parametrize("G_", [1, 3])
def test_chunk_edges_match_float64_restatement(device, G_):
    """Per task, tensors one element long, one short of a chunk, a chunk, one over, two chunks and one, four chunks."""
    params, grads = _edge_case(G_, [(k,) for k in EDGE_NUMEL], 20 + G_)
    p1, g1, norm = _run(device, params, grads)
    _check_restatement(params, grads, p1, g1, norm, G_)


def test_32_tensors_and_no_more(device):
    """32 tensors (OPT_MAX_TENSORS) work; 33 are refused with nothing written."""
    from merlin import _native as nat

    shapes = [(EDGE_NUMEL[i % len(EDGE_NUMEL)] + i // len(EDGE_NUMEL),) for i in range(32)]
    params, grads = _edge_case(2, shapes, 30)
    p1, g1, norm = _run(device, params, grads)
    _check_restatement(params, grads, p1, g1, norm, 2)

    p = [torch.from_numpy(x.copy()).to(device) for x in params] + [torch.ones(2, 7, device=device)]
    g = [torch.from_numpy(x.copy()).to(device) for x in grads] + [torch.ones(2, 7, device=device)]
    norm_out = torch.full((2,), -3.0, device=device)
    with pytest.raises(ValueError):
        nat.group_clip_sgd(p, g, LR, MAX_NORM, norm_out=norm_out)
    torch.cuda.synchronize()
    for a, b in zip(p + g, params + [np.ones((2, 7), np.float32)] + grads + [np.ones((2, 7), np.float32)]):
        assert (a.cpu().numpy().view(np.int32) == b.view(np.int32)).all()
    assert (norm_out == -3.0).all()


def test_empty_tensor_is_refused(device):
    """A tensor without elements per task is refused, in any position, with nothing written."""
    from merlin import _native as nat

    for pos in (0, 1, 2):
        p = [torch.ones(3, 5, device=device), torch.ones(3, 1025, device=device)]
        p.insert(pos, torch.ones(3, 0, device=device))
        g = [torch.full_like(x, 2.0) for x in p]
        norm_out = torch.full((3,), -3.0, device=device)
        with pytest.raises(ValueError):
            nat.group_clip_sgd(p, g, LR, MAX_NORM, norm_out=norm_out)
        torch.cuda.synchronize()
        assert all((x == 1.0).all() for x in p) and all((x == 2.0).all() for x in g) and (norm_out == -3.0).all()
