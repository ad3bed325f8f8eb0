"""CPU: bench.py's --dump-outputs writer (dump_outputs): float32 / float64 .npy files, one per name, and a fixed
sample of an array larger than its share of the dump's budget, the same elements on every call."""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parse_has_full_and_dump_outputs_off_by_default(bench, monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 2
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_writes_float_arrays(bench, tmp_path):
    import torch

    arrays = {"ints": torch.arange(12, dtype=torch.int64).reshape(3, 4), "f64": np.linspace(0, 1, 5),
              "f32": torch.ones(2, 3), "scalars": [1.5, 2.5]}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["f32.npy", "f64.npy", "ints.npy", "scalars.npy"]
    ints = np.load(tmp_path / "out" / "ints.npy")
    assert ints.dtype == np.float32 and ints.shape == (3, 4) and (ints == np.arange(12).reshape(3, 4)).all()
    f64 = np.load(tmp_path / "out" / "f64.npy")
    assert f64.dtype == np.float64 and (f64 == np.linspace(0, 1, 5)).all()
    assert np.load(tmp_path / "out" / "scalars.npy").dtype == np.float64  # Python floats keep their precision


def test_dump_samples_what_exceeds_the_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 400)  # 400 B = 100 float32 per array
    big = np.arange(1000, dtype=np.float32).reshape(10, 100)
    small = np.arange(50, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (100,) and (a == b).all()  # the same sample both times
    assert (np.diff(a) > 0).all() and set(a.tolist()) <= set(range(1000))  # distinct elements of big, in order
    assert (np.load(tmp_path / "a" / "small.npy") == small).all()
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 2 * 400 + 2 * 128  # the budget + the .npy headers
