import os
import sys

import pytest

# MIOpen (the reference-structured F.conv2d paths the parity tests compare against): heuristic
# solver choice instead of a per-shape Find that compiles and times every candidate kernel
# (minutes for a new batch shape on a fresh box).  Same fp32 convolutions.
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
os.environ.setdefault("MIOPEN_LOG_LEVEL", "3")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ppo-2dgrid_amd")
ORACLE = os.path.join(REPO, "oracle")
GOLDEN = os.path.join(REPO, "tests", "golden")
for p in (PKG, ORACLE):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP device); parity tests proper")


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    cache = {}

    def load(name):
        if name not in cache:
            path = os.path.join(GOLDEN, name + ".npz")
            if os.path.exists(path):
                cache[name] = np.load(path, allow_pickle=False)
            else:  # a fixture over the committed-file size limit: NAME.partKK.npz (tests/golden/parts.py)
                import importlib.util

                spec = importlib.util.spec_from_file_location("golden_parts", os.path.join(GOLDEN, "parts.py"))
                parts = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(parts)
                cache[name] = parts.load_parts(os.path.join(GOLDEN, name))
        return cache[name]

    return load


@pytest.fixture(scope="session")
def oracle():
    import oracle as O  # test infrastructure: the checker

    O.build()
    return O


def gpu_available():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="session")
def device():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a visible HIP device")
    return torch.device("cuda:0")
