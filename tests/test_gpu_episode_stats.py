"""GPU: merlin_episode_class_stats (csrc/merlin_epstats.hip) on synthetic rollouts, no env.

Counts and length sums are integers far below 2^53: exact.  A return sum s of `count` fp64 terms, in whatever order
the kernel adds them, satisfies |s - exact| <= (count - 1) u sum|x| + O(u^2) with u = 2^-53 (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2); the tests hold it to count * 2^-53 * sum|x| against math.fsum (the
exactly rounded sum).  The squares x * x are rounded once on both sides (IEEE multiplication, no contraction), so the
same bound holds for their sum."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def synth(T, N, n_classes, seed, empty_class=None, idle_class=None):
    """done ~20 %, returns of mixed sign and magnitude, lengths 1..400.  empty_class: assigned to no env;
    idle_class: has envs but no finished episode."""
    rs = np.random.RandomState(seed)
    pool = [c for c in range(n_classes) if c != empty_class]
    cls = np.array([pool[i % len(pool)] for i in rs.permutation(N)], dtype=np.uint8) if N else np.zeros(0, np.uint8)
    done = (rs.rand(T, N) < 0.2).astype(np.float32)
    if idle_class is not None:
        done[:, cls == idle_class] = 0.0
    ret = (rs.randn(T, N) * np.exp(rs.randn(T, N) * 3.0)).astype(np.float64)
    length = rs.randint(1, 401, size=(T, N)).astype(np.int32)
    return done, ret, length, cls


def host_stats(done, ret, length, cls, n_classes):
    """Per class: (count, fsum(x), fsum(x*x), sum of lengths, sum|x|, sum x*x) -- the exactly rounded references."""
    out = []
    for c in range(n_classes):
        m = (done != 0) & (cls == c)[None, :] if done.size else np.zeros(done.shape, bool)
        x = ret[m]
        out.append((int(m.sum()), math.fsum(x), math.fsum(x * x), int(length[m].astype(np.int64).sum()),
                    math.fsum(np.abs(x)), math.fsum(x * x)))
    return out


def run(device, done, ret, length, cls, n_classes, out=None, accumulate=False):
    from merlin import _native as nat

    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return nat.episode_class_stats(t(done), t(ret), t(length), t(cls), n_classes, out=out, accumulate=accumulate)


def check(got, ref):
    got = got.cpu().numpy()
    for c, (cnt, s1, s2, sl, a1, a2) in enumerate(ref):
        print(f"class {c}: count {got[c, 0]:.0f}/{cnt} sum err {abs(got[c, 1] - s1):.3e} (bound {cnt * U * a1:.3e}) "
              f"sq err {abs(got[c, 2] - s2):.3e} (bound {cnt * U * a2:.3e}) length {got[c, 3]:.0f}/{sl}")
        assert got[c, 0] == cnt and got[c, 3] == sl, c
        assert abs(got[c, 1] - s1) <= cnt * U * a1, c
        assert abs(got[c, 2] - s2) <= cnt * U * a2, c


@pytest.mark.parametrize("T,N", [(7, 130), (3, 4097)], ids=["7x130", "3x4097"])
def test_against_host(device, T, N):
    """T = 7, N = 130: one partial column tile.  T = 3, N = 4096 + 1: 17 column tiles, the last with one env."""
    n_classes = 5
    done, ret, length, cls = synth(T, N, n_classes, seed=T * 1000 + N, empty_class=3, idle_class=1)
    ref = host_stats(done, ret, length, cls, n_classes)
    assert ref[3][0] == 0 and (cls == 3).sum() == 0  # no env
    assert ref[1][0] == 0 and (cls == 1).sum() > 0  # envs, no finished episode
    assert all(ref[c][0] > 0 for c in (0, 2, 4))
    a = run(device, done, ret, length, cls, n_classes)
    assert a.shape == (n_classes, 4) and a.dtype == torch.float64
    check(a, ref)
    assert (a[3] == 0).all() and (a[1] == 0).all()
    # a second launch: the same bits
    b = run(device, done, ret, length, cls, n_classes)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # accumulate on top of the first result: counts and lengths double exactly, the sums stay within the bound of
    # 2 * count terms
    acc = a.clone()
    run(device, done, ret, length, cls, n_classes, out=acc, accumulate=True)
    assert torch.equal(acc[:, 0], 2 * a[:, 0]) and torch.equal(acc[:, 3], 2 * a[:, 3])
    check(acc, [(2 * cnt, 2 * s1, 2 * s2, 2 * sl, 2 * a1, 2 * a2) for cnt, s1, s2, sl, a1, a2 in ref])


def test_many_step_slabs(device):
    """T = 300 at N = 1100: 5 column tiles (the last partial) x 50 slabs of 6 rows, and all 8 classes."""
    done, ret, length, cls = synth(300, 1100, 8, seed=9)
    check(run(device, done, ret, length, cls, 8), host_stats(done, ret, length, cls, 8))


def test_empty_rollout_gives_zeros(device):
    from merlin import _native as nat

    for T, N in ((0, 130), (0, 0)):
        done, ret, length, cls = synth(T, N, 5, seed=1)
        out = torch.full((5, 4), 7.0, dtype=torch.float64, device=device)
        run(device, done, ret, length, cls, 5, out=out)
        assert (out == 0).all(), (T, N)
        out.fill_(3.0)
        run(device, done, ret, length, cls, 5, out=out, accumulate=True)
        assert (out == 3.0).all(), (T, N)
    with pytest.raises(ValueError):
        nat.episode_class_stats(torch.zeros((2, 4), device=device), torch.zeros((2, 4), dtype=torch.float64,
                                device=device), torch.zeros((2, 4), dtype=torch.int32, device=device),
                                torch.zeros(4, dtype=torch.uint8, device=device), 9)


def test_classes_beyond_n_classes_are_ignored(device):
    done, ret, length, cls = synth(5, 200, 5, seed=4)
    ref = host_stats(done, ret, length, cls, 3)
    check(run(device, done, ret, length, cls, 3), ref)


def test_more_column_tiles_than_one_round(device):
    """T = 2, N = 256 * 1024 + 257: 1,026 column tiles against a workspace of 1,024 block partials, so two rounds
    (1,024 tiles, then 2 with the last holding one env), the second folded onto the first; one step slab each."""
    T, N, n_classes = 2, 256 * 1024 + 257, 5
    assert -(-N // 256) == 1024 + 2 and N % 256 == 1
    done, ret, length, cls = synth(T, N, n_classes, seed=11)
    done[:, -1], cls[-1] = 1.0, 2  # the env alone in the last tile finishes, twice
    ref = host_stats(done, ret, length, cls, n_classes)
    assert all(r[0] > 0 for r in ref)
    late = host_stats(done[:, 256 * 1024:], ret[:, 256 * 1024:], length[:, 256 * 1024:], cls[256 * 1024:], n_classes)
    assert all(r[0] > 0 for r in late)  # every class has episodes in the second round
    a = run(device, done, ret, length, cls, n_classes)
    check(a, ref)
    b = run(device, done, ret, length, cls, n_classes)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # into a prefilled `out`: the first round overwrites, the second adds; accumulate adds both
    c = run(device, done, ret, length, cls, n_classes, out=torch.full((n_classes, 4), 7.0, dtype=torch.float64,
                                                                       device=device))
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    acc = a.clone()
    run(device, done, ret, length, cls, n_classes, out=acc, accumulate=True)
    assert torch.equal(acc[:, 0], 2 * a[:, 0]) and torch.equal(acc[:, 3], 2 * a[:, 3])
    check(acc, [(2 * cnt, 2 * s1, 2 * s2, 2 * sl, 2 * a1, 2 * a2) for cnt, s1, s2, sl, a1, a2 in ref])
