"""mrt_update_instances_device without a device: the entry point is exported with the header's argument types, refuses a null
context, and the per-instance arithmetic it shares with the host path (csrc/instance_math.h: inverse transform, world box) gives
the host path's results bit for bit (csrc/host/instance_math_test.cpp, compiled for the CPU)."""
import ctypes as C
import os
import re
import subprocess

from messyerraytracer_amd import build as mbuild, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mrt_hip.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_entry_point_is_declared_exported_and_bound():
    text = _header()
    decl = re.search(r"int\s+mrt_update_instances_device\s*\(([^)]*)\)\s*;", text)
    assert decl, "mrt_update_instances_device is not declared in include/mrt_hip.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["mrt_ctx *ctx", "const mrt_instance *instances", "uint32_t n_instances", "uint32_t flags"], args
    m = re.search(r"MRT_BUILD_INSTANCES_ON_DEVICE\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and (1 << int(m.group(1))) == capi.BUILD_INSTANCES_ON_DEVICE == 32
    assert "mrt_update_instances_device" in capi.SYMBOLS
    L = capi.load()
    fn = L.mrt_update_instances_device
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    assert fn.restype is C.c_int
    assert set(capi.TLAS_FORMS) == {"radix", "ploc", "sah"}
    assert capi.TLAS_FORMS["ploc"] == capi.BUILD_PLOC and capi.TLAS_FORMS["sah"] == capi.BUILD_SAH and capi.TLAS_FORMS["radix"] == 0


def test_null_context_is_refused():
    L = capi.load()
    for flags in (0, capi.BUILD_INSTANCES_ON_DEVICE, capi.BUILD_INSTANCES_ON_DEVICE | capi.BUILD_SAH, 0xFFFFFFFF):
        assert L.mrt_update_instances_device(None, None, 0, flags) == capi.ERR_INVALID
        assert L.mrt_update_instances_device(None, None, 64, flags) == capi.ERR_INVALID


def test_shared_instance_math_matches_the_host_path_bit_for_bit():
    exe = mbuild.build_instance_math_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout[-4000:]
    n = int(re.search(r"(\d+) checks hold", r.stdout).group(1))
    assert n > 50000
