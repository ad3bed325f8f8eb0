"""CPU: the tie resolver of tests/grad64_ref.py on the gradient fixture alone.

The float64 gradient and the tie groups are built from `update_grad_ref` at the fixture's weights (the first
minibatch, the reference's normalised advantages and returns).  Planted subsets of group flips plus Gaussian noise of
relative norm 1e-6 per tensor must come back exactly, with a remainder under REL; a perturbation that is NOT a tie
vector (2e-4 of a random direction on actor.0.weight, well inside the old tie envelope) must leave a remainder over
REL; the reference's own fp32 gradient must resolve with zero flips."""
import numpy as np
import pytest
import torch

import grad64_ref as G

NOISE = 1e-6
NOISE_BOUND = 1.5 * NOISE  # with the right flips the remainder is the planted noise itself, far under REL


@pytest.fixture(scope="module")
def ref(golden, oracle):
    g = golden("update_grad_ref")
    B, MB, _ = (int(x) for x in g["cfg"])
    names = [str(n) for n in g["param_names"]]
    weights = [torch.from_numpy(g[f"p0_{i}"]) for i in range(len(names))]
    r = G.grad64(names, weights, G.fixture_frames(g, oracle, golden), g["actions"], g["perms"][0][:MB],
                 g["adv_norm"], g["returns"], g["logp"], g["hparams"])
    print(G.describe_ties(r))
    return g, r


def _rel(diff, ref):
    return [float(d.norm()) / float(t.norm()) for d, t in zip(diff, ref.grads)]


def _noise(ref, gen, scale=NOISE):
    out = []
    for t in ref.grads:
        n = torch.randn(t.shape, generator=gen, dtype=torch.float64)
        out.append(n * (scale * float(t.norm()) / float(n.norm())))
    return out


def test_fixture_has_ties_and_groups(ref):
    _, r = ref
    assert r.coef == 1.0  # the first step's norm is under clip_grad_norm_'s 0.5
    assert len(r.ties) >= len(r.groups) >= 2
    assert sorted(i for m in r.groups for i in m) == list(range(len(r.ties)))
    for k, m in enumerate(r.groups):  # a group's vector is the sum of its members'
        assert torch.equal(r.gdeltas[k], r.deltas[m].sum(0))
        assert float(r.gdeltas[k].norm()) > 0.0
    # the envelope of the old bound is the per-tensor sum of the ties' own norms
    env = [sum(float(t.norm()) for t in col) for col in zip(*(G.unflat(d, r.grads) for d in r.deltas))]
    assert np.allclose(env, r.env, rtol=1e-12, atol=0.0)
    assert max(e / float(t.norm()) for e, t in zip(r.env, r.grads)) > 1e-3  # the slack the old bound gave away


def test_planted_flips_come_back_exactly(ref):
    _, r = ref
    K = len(r.groups)
    gen = torch.Generator().manual_seed(7)
    subsets = [[], list(range(K))] + [[k] for k in range(K)]
    for sub in subsets:
        planted = np.zeros(K, dtype=bool)
        planted[sub] = True
        diff = G.unflat(r.gdeltas[torch.from_numpy(planted)].sum(0), r.grads)
        diff = [d + n for d, n in zip(diff, _noise(r, gen))]
        flips, f, rem = G.resolve(diff, r.gdeltas)
        assert (flips == planted).all(), (sub, np.nonzero(flips)[0].tolist(), f.tolist())
        worst = max(_rel(rem, r))
        assert worst <= NOISE_BOUND <= G.REL, (sub, worst)


def test_non_tie_perturbation_fails_resolved_bound_but_passes_envelope(ref):
    """What the old test could not see: 2e-4 |g| of a random direction on actor.0.weight alone."""
    _, r = ref
    gen = torch.Generator().manual_seed(11)
    i = r.names.index("actor.0.weight")
    diff = _noise(r, gen)
    n = torch.randn(r.grads[i].shape, generator=gen, dtype=torch.float64)
    diff[i] = diff[i] + n * (2e-4 * float(r.grads[i].norm()) / float(n.norm()))
    d = _rel(diff, r)
    assert all(d[j] * float(r.grads[j].norm()) <= G.REL * float(r.grads[j].norm()) + r.env[j]
               for j in range(len(d)))  # the old envelope bound holds on every tensor
    flips, f, rem = G.resolve(diff, r.gdeltas)
    res = _rel(rem, r)
    assert res[i] > 10 * G.REL, res[i]  # the resolved bound does not
    assert all(res[j] <= G.REL for j in range(len(res)) if j != i)
    # and a real flip on top of it is still identified
    diff2 = [a + b for a, b in zip(diff, G.unflat(r.gdeltas[0], r.grads))]
    flips2, _, rem2 = G.resolve(diff2, r.gdeltas)
    assert flips2.tolist() == [k == 0 for k in range(len(r.groups))]
    assert _rel(rem2, r)[i] > 10 * G.REL


def test_reference_gradient_resolves_with_zero_flips(ref):
    g, r = ref
    gr = [torch.from_numpy(g[f"grad{i}"]).double() for i in range(len(r.names))]
    flips, f, rem = G.resolve([a - b for a, b in zip(gr, r.grads)], r.gdeltas)
    res = _rel(rem, r)
    for name, x in zip(r.names, res):
        print(f"{name:36s} reference vs float64, resolved {x:.2e}")
    assert not flips.any(), (np.nonzero(flips)[0].tolist(), f.tolist())
    assert max(res) <= G.REL, res
