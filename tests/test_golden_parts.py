"""CPU: fixtures stored in parts (tests/golden/parts.py) come back bit for bit, and every committed fixture file
stays under the 1 MiB limit for a committed file."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def parts():
    spec = importlib.util.spec_from_file_location("golden_parts", os.path.join(GOLDEN, "parts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parts_round_trip(parts, tmp_path, monkeypatch):
    monkeypatch.setattr(parts, "PART_BYTES", 1000)
    rs = np.random.RandomState(0)
    arrays = {"small": rs.rand(7).astype(np.float32), "big": rs.rand(13, 101).astype(np.float32),  # 5252 B: 6 chunks
              "names": np.array(["a.weight", "b.bias"]), "half": rs.rand(3, 5).astype(np.float16),
              "exact": rs.rand(250).astype(np.float32)}  # exactly PART_BYTES: not cut
    stem = str(tmp_path / "fx")
    n = parts.save_parts(stem, arrays)
    assert n == len(parts.part_files(stem)) >= 7
    back = parts.load_parts(stem)
    assert list(back) == list(arrays)
    for k, a in arrays.items():
        assert back[k].dtype == a.dtype and back[k].shape == a.shape and back[k].tobytes() == a.tobytes(), k
    # saving again with fewer parts leaves no stale part behind
    monkeypatch.setattr(parts, "PART_BYTES", 1 << 20)
    assert parts.save_parts(stem, arrays) == 1 and len(parts.part_files(stem)) == 1
    with pytest.raises(FileNotFoundError):
        parts.load_parts(str(tmp_path / "absent"))


def test_committed_fixture_files_are_under_one_mib(golden):
    for f in os.listdir(GOLDEN):
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= 1 << 20, f
    g = golden("update_grad_ref")  # the fixture stored in parts
    assert g["p0_12"].shape == (512, 576) and g["p0_12"].dtype == np.float32
