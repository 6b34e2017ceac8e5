import functools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def gpu_present() -> bool:
    """Whether torch sees a GPU, asked in a fresh interpreter: torch brings its own HIP runtime, and once libmrt_hip.so
    has loaded the system's into this process torch's answer here is no longer to be trusted."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.split()[-1] == "True"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def built():
    """Everything compiled (idempotent; the GPU box uses the prebuilt .so files)."""
    import __graft_entry__ as g
    g.build()
    return True


@pytest.fixture(scope="session")
def ctx(built):
    from messyerraytracer_amd import capi
    c = capi.Context(0)
    yield c
    c.close()
