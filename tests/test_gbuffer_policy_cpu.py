"""The launch policy of G-buffer reflection casts without a device (csrc/host/record_policy_test.cpp, launch_policy.cpp alone): the
plan of a reflection cast of as many rays, row by row; a primary grid's plans and states untouched by G-buffer casts between its
frames; and the labels of the family's seven forms."""
import subprocess

from messyerraytracer_amd import build as mbuild


def test_gbuffer_policy_driver():
    exe = mbuild.build_record_policy_test()
    r = subprocess.run([exe, "gbuffer"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
