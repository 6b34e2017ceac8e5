"""Shadow casts without a device: the library exports mrt_cast_shadows / mrt_cast_grid_shadows, mrt_light is the 32-byte struct the
binding declares, the calls reject bad arguments before any device work, and the launch policy plans shadow casts as unsorted
non-coherent any-hit batches that never touch the primary grid's state (csrc/host/shadow_policy_test.cpp, launch_policy.cpp alone)."""
import ctypes as C
import subprocess

import numpy as np

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import types as T


def test_exports_and_struct_size():
    L = capi.load()
    for s in ("mrt_cast_shadows", "mrt_cast_grid_shadows"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert L.mrt_struct_size(4) == 32 == T.LIGHT.itemsize
    assert L.mrt_struct_size(5) == 0


def test_null_context_is_invalid():
    L = capi.load()
    lights = np.zeros(1, dtype=T.LIGHT)
    assert L.mrt_cast_shadows(None, C.c_void_p(16), C.c_void_p(16), 1, lights.ctypes.data_as(C.c_void_p), 1,
                              C.c_void_p(16), 0xFFFFFFFF, 0) == capi.ERR_INVALID
    cam = capi.Camera()
    assert L.mrt_cast_grid_shadows(None, C.byref(cam), 4, 4, 0, 4, C.c_void_p(16), lights.ctypes.data_as(C.c_void_p), 1,
                                   C.c_void_p(16), 0xFFFFFFFF, 0) == capi.ERR_INVALID


def test_shadow_policy_driver():
    exe = mbuild.build_shadow_policy_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
