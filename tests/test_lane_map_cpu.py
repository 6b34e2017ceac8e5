"""The lane map in two parts (csrc/lane_map.h: a group's tile once per wave, the lane's pixel per lane) against the one function it
replaces, restated in csrc/host/lane_map_test.cpp: every lane of every group for random grids, tile shapes, tile orders, schedules
with pieces and quarter modes, widths and row counts of 1, 7, 8, 9, 4095 and 4097, and a tile count above 2^32 -- a stand-alone host
program, built twice: plain, and under AddressSanitizer + UndefinedBehaviorSanitizer.  Nothing is loaded into Python."""
import re
import subprocess

import pytest

from messyerraytracer_amd import build as mbuild


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_two_part_lane_map_is_the_one_function_map(sanitize):
    exe = mbuild.build_lane_map_test(sanitize=sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout[-4000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, report
    for bad in ("runtime error", "AddressSanitizer", "LeakSanitizer"):
        assert bad not in report, report
    assert int(re.search(r"(\d+) checks hold", r.stdout).group(1)) > 10_000_000
