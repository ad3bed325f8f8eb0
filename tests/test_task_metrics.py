"""CPU: merlin.metrics.task_metrics against the reference's src/metrics/task_metrics.py outputs
(tests/golden/task_metrics_ref.npz, made by tests/golden/make_fewshot_golden.py): the same float64 numpy
arithmetic, so 1e-12 relative."""
import numpy as np
import pytest

CASES = ("a", "b", "c")  # (40, 3) vs (25, 3); a 1-D pair; a constant column (the 1e-8 std floor)


@pytest.mark.parametrize("case", CASES)
def test_compare_two_feature_sets_matches_reference(golden, case):
    from merlin.metrics.task_metrics import compare_two_feature_sets

    fx = golden("task_metrics_ref")
    out = compare_two_feature_sets(fx[f"{case}_x"], fx[f"{case}_y"])
    keys = [str(k) for k in fx["keys"]]
    assert sorted(out) == sorted(keys)
    for k, ref in zip(keys, fx[f"{case}_out"]):
        assert np.isfinite(out[k]) and abs(out[k] - ref) <= 1e-12 * max(1.0, abs(ref)), (case, k, out[k], ref)


def test_parts_are_the_stated_formulas(golden):
    from merlin.metrics import task_metrics as tm

    fx = golden("task_metrics_ref")
    x, y = fx["a_x"], fx["a_y"]
    m, s = tm.compute_mean_std(x)
    assert m.shape == s.shape == (3,) and np.allclose(s, x.std(axis=0) + 1e-8, rtol=0, atol=0)
    assert tm.compute_mean_std(fx["b_x"])[0].shape == (1,)  # 1-D samples are one feature
    assert tm.compute_mean_std(fx["c_x"])[1][1] == 1e-8  # constant column: the floor alone
    assert tm.kl_diag_gaussians(m, s, m, s) == 0.0 and tm.js_diag_gaussians(m, s, m, s) == 0.0
    # the longer sample is truncated after sorting
    u, v = np.array([3.0, 1.0, 2.0, 100.0]), np.array([1.5, 0.5])
    assert tm.wasserstein_1d(u, v) == np.mean([abs(1.0 - 0.5), abs(2.0 - 1.5)])
    assert tm.wasserstein_1d(u, []) == 0.0
    assert tm.wasserstein_mean(x, y) == np.mean([tm.wasserstein_1d(x[:, d], y[:, d]) for d in range(3)])
    pairs = tm.compare_task_feature_dict({"p": x, "q": y, "r": x + 1.0})
    assert list(pairs) == [("p", "q"), ("p", "r"), ("q", "r")]
    assert pairs[("p", "q")] == tm.compare_two_feature_sets(x, y)
