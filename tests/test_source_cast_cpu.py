"""The host side of the record-driven casts without a device (csrc/source_cast.h, csrc/host/source_cast_data.cpp): per family the
refusals in the header's order and the edges of every range, the kernels' arguments, the jumps against stepping the generator, the seed
of a row band, the batch each entry point sets (csrc/host/source_cast_data_test.cpp).  A program of its own; nothing of it is loaded
into this process."""
import subprocess

import pytest

from messyerraytracer_amd import build as mbuild


@pytest.mark.parametrize("sanitize", [False, True])
def test_source_cast_data_driver(sanitize):
    """With and without AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = mbuild.build_source_cast_data_test(sanitize=sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_the_seed_rule_is_written_once():
    """pixel0 * 1009 + frame * 6529 + 7 stands in source_cast.h alone among the host's sources (the kernels and the test programs
    restate it to be held to it)."""
    import glob
    import os
    named = []
    for pat in ("*.h", "*.hip", "host/*.cpp", "host/*.hpp"):
        for path in glob.glob(os.path.join(mbuild.CSRC, pat)):
            name = os.path.basename(path)
            if name.endswith("_test.cpp") or name.endswith("_kernel.h") or name.endswith("kernels.hip"):
                continue
            with open(path) as f:
                if "1009u" in f.read():
                    named.append(name)
    assert named == ["source_cast.h"], named
