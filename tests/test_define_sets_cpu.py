"""Every define set the walks are built with still compiles: the C++ and the operand lists of the assembly blocks of kernels.hip,
device side only, nothing assembled or linked (-fsyntax-only).  A switch build that no test builds rots unseen: the four-wide walk
(MRT_WITH_QUAD) did not compile for several commits while its GPU tests skipped for want of the kernel."""
import os
import shutil
import subprocess

import pytest

from messyerraytracer_amd import build

DEFINE_SETS = [[], ["-DMRT_WITH_QUAD"], ["-DMRT_ROWS_POPFETCH=1"], ["-DMRT_ROWS_PKSLAB=1"], ["-DMRT_WITH_QUAD", "-DMRT_ROWS_POPFETCH=1"]]


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.mark.parametrize("defines", DEFINE_SETS, ids=lambda d: " ".join(d) or "default")
def test_walks_compile_with(defines):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc] + build.FLAGS + defines + ["--cuda-device-only", "-fsyntax-only", "kernels.hip"],
                       capture_output=True, text=True, cwd=build.CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
