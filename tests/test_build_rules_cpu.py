"""The rules the host and the device scene builders share (csrc/build_rules.h: the triangle of three vertices, its box, the re-basing
of a ref, the widening of a binary node to 4 and 8 children, the grid of an 8-wide node) against the host path's text they replaced,
restated in csrc/host/build_rules_test.cpp: bit for bit on random inputs and on zero-area triangles, +-0 and denormals, coordinates
at +-FLT_MAX, boxes of zero extent, extents at the ends of the exponent range and of exactly 254 steps, NaN and infinite boxes,
nodes of two leaves, chains that fill every slot, refs around the sentinel -- a stand-alone host program, built twice: plain, and
under AddressSanitizer + UndefinedBehaviorSanitizer.  Nothing is loaded into Python."""
import re
import subprocess

import pytest

from messyerraytracer_amd import build as mbuild


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_shared_build_rules_are_the_host_paths_text(sanitize):
    exe = mbuild.build_build_rules_test(sanitize=sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout[-4000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, report
    for bad in ("runtime error", "AddressSanitizer", "LeakSanitizer"):
        assert bad not in report, report
    assert int(re.search(r"(\d+) checks hold", r.stdout).group(1)) > 100_000
    assert int(re.search(r"(\d+) boxes refused alike", r.stdout).group(1)) >= 60
