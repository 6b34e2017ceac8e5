"""Reflection casts without a device: the library exports mrt_cast_reflections / mrt_cast_grid_reflections, the calls reject a null
context and bad arguments before any device work, and the launch policy plans reflection casts as unsorted non-coherent closest-hit
batches that never touch the primary grid's state (csrc/host/reflection_policy_test.cpp, launch_policy.cpp alone)."""
import ctypes as C
import math
import subprocess

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi

P = C.c_void_p(16)  # a pointer no call may dereference: every case below fails its checks first


def test_exports():
    L = capi.load()
    for s in ("mrt_cast_reflections", "mrt_cast_grid_reflections"):
        assert hasattr(L, s) and s in capi.SYMBOLS


def test_null_context_is_invalid():
    L = capi.load()
    assert L.mrt_cast_reflections(None, P, P, 1, None, 10.0, P, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    cam = capi.Camera()
    assert L.mrt_cast_grid_reflections(None, C.byref(cam), 4, 4, 0, 4, P, None, 10.0, P, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID


def test_bad_arguments_without_a_context_are_invalid():
    """(With a context, every bad argument is checked before the scene and before any device work: test_reflections_gpu.py.)"""
    L = capi.load()
    cam = capi.Camera()
    for dist in (math.nan, math.inf, 0.0, -1.0):
        assert L.mrt_cast_reflections(None, P, P, 1, None, dist, P, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
        assert L.mrt_cast_grid_reflections(None, C.byref(cam), 4, 4, 0, 4, P, None, dist, P, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    assert L.mrt_cast_reflections(None, None, None, 1, None, 1.0, None, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    assert L.mrt_cast_grid_reflections(None, None, 4, 4, 3, 2, None, None, 1.0, None, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID


def test_reflection_policy_driver():
    exe = mbuild.build_reflection_policy_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
