"""Reflection casts without a device: the library exports mrt_cast_reflections / mrt_cast_grid_reflections, the calls reject a null
context and bad arguments before any device work, and the launch policy plans reflection casts as unsorted non-coherent closest-hit
batches that never touch the primary grid's state (csrc/host/record_policy_test.cpp, launch_policy.cpp alone); the numpy
restatement of the formula (messyerraytracer_amd/reflection.py, what the GPU tests hold the kernels to byte for byte) against float64
within a derived bound, and its exact properties."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import reflection as R
import source_edge_cases as E

F = np.float32

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
    exe = mbuild.build_record_policy_test()
    r = subprocess.run([exe, "reflection"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


# ---- the restatement.  GLSL's reflect has no stated rounding, so there is no recording to equal: the direction is held to float64
# and everything that is exact is held exactly.

@pytest.fixture(scope="module")
def cases():
    d, n, kind = E.reflection_inputs()
    pos = np.random.default_rng(5).uniform(-5, 5, size=d.shape).astype(F)
    rays, flipped = R.reflection_rays(d, pos, n, np.ones(d.shape[0], dtype=bool), 25.0)
    return d, n, kind, pos, rays, flipped


def r32(x):
    """a float64 result rounded once to float32 (exact for one +, -, * of float32 operands: 53 >= 2 * 24 + 2), kept as float64"""
    return np.asarray(x, dtype=np.float64).astype(F).astype(np.float64)


def dot32(n, d):
    """(nx*dx + ny*dy) + nz*dz, each operation in float64 rounded once: the float32 sum by another route"""
    n, d = n.astype(np.float64), d.astype(np.float64)
    return r32(r32(r32(n[:, 0] * d[:, 0]) + r32(n[:, 1] * d[:, 1])) + r32(n[:, 2] * d[:, 2]))


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_inputs_cover_what_they_name(cases):
    d, n, kind, _, _, flipped = cases
    assert d.shape == (E.N, 3) and set(kind) == {"unit", "non-unit", "huge", "orthogonal", "zero-normal", "signed-zero"}
    c = dot32(n, d)
    assert flipped[kind == "unit"].any() and (~flipped[kind == "unit"]).any()            # back and front faces
    o = kind == "orthogonal"
    assert (c[o] == 0).all() and np.signbit(c[o]).any() and (~np.signbit(c[o])).any()    # n . d evaluates to +0 and to -0
    assert o.sum() >= 100
    assert (np.abs(np.linalg.norm(d[kind == "huge"].astype(np.float64), axis=1) / 1e18 - 1) < 1e-6).all()
    assert not n[kind == "zero-normal"].any() and np.signbit(n[kind == "zero-normal"]).any()
    assert (np.signbit(d) & (d == 0)).any() and (np.signbit(n) & (n == 0)).any()


def test_direction_is_within_the_derived_bound_of_float64(cases):
    """dir = d - 2 (n . d) n.  In float32 the dot product rounds each term at most three times (its product and two sums), the doubling
    is exact, k * n_i rounds once and the subtraction once: |dir32_i - dir64_i| <= u (|dir_i| + |k n_i| + 6 |n_i| S) with
    u = 2^-24 and S = sum |n_j d_j|, plus 1 % for the second-order terms.  Derived, not measured."""
    d, n, _, _, rays, _ = cases
    d64, n64 = d.astype(np.float64), n.astype(np.float64)
    k = 2.0 * (n64 * d64).sum(axis=1)
    want = d64 - k[:, None] * n64
    S = np.abs(n64 * d64).sum(axis=1)
    bound = 2.0 ** -24 * (np.abs(want) + np.abs(k[:, None] * n64) + 6.0 * np.abs(n64) * S[:, None]) * 1.01
    err = np.abs(rays["direction"].astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("largest error / bound: %.3f" % worst)
    assert (err <= bound).all(), worst
    assert worst > 0.05   # (the bound is not vacuous on these inputs: some case uses a real part of it)


def test_direction_ignores_the_sign_of_the_normal(cases):
    """Negation is exact, so n and -n give the same faced normal, the same k and the same ray -- wherever the sum is not zero.  Where it
    is +-0 neither normal is turned (the origins then lie on opposite sides) and dir is d by value, its zeros' signs as the next test
    states them."""
    d, n, _, pos, rays, _ = cases
    other, _ = R.reflection_rays(d, pos, -n, np.ones(d.shape[0], dtype=bool), 25.0)
    nonzero = dot32(n, d) != 0
    assert nonzero.sum() > 3000
    np.testing.assert_array_equal(bits(other["direction"])[nonzero], bits(rays["direction"])[nonzero])
    np.testing.assert_array_equal(bits(other["origin"])[nonzero], bits(rays["origin"])[nonzero])
    np.testing.assert_array_equal(other["direction"][~nonzero], rays["direction"][~nonzero])


def test_direction_is_d_where_the_dot_product_is_zero(cases):
    """n . d evaluating to +0 or -0 gives k = +-0 and k * n_i = +-0: d_i - (+-0) is d_i bit for bit -- but for one IEEE corner: a d_i
    that is itself -0.0 comes back +0.0 when k * n_i is -0.0 ((-0) - (-0) = +0).  The inputs hold that corner; everything else is
    held by its bits, the corner by its value and by the sign it must then have."""
    d, n, kind, _, rays, _ = cases
    zero = dot32(n, d) == 0
    assert zero[kind == "orthogonal"].all() and zero[kind == "zero-normal"].all()
    got, want = rays["direction"][zero], d[zero]
    np.testing.assert_array_equal(got, want)
    neg_zero = np.signbit(want) & (want == 0)
    np.testing.assert_array_equal(bits(got)[~neg_zero], bits(want)[~neg_zero])
    nz = n[zero].copy()
    c = dot32(n[zero], d[zero])
    k_times_n_negative = (np.signbit(c)[:, None] ^ np.signbit(nz))     # the sign of (+-0) * n_i (no flip: c is not > 0)
    np.testing.assert_array_equal(np.signbit(got)[neg_zero], ~k_times_n_negative[neg_zero])
    assert (neg_zero & k_times_n_negative).any() and (neg_zero & ~k_times_n_negative).any()


def test_flip_exactly_when_the_float32_sum_is_positive(cases):
    d, n, _, _, _, flipped = cases
    c = dot32(n, d)
    np.testing.assert_array_equal(flipped, c > 0)
    assert (c > 0).any() and (c < 0).any() and (c == 0).any()
    assert (np.abs(c[c != 0]).min()) < 1e-3    # (near-grazing pairs on both sides are among the random ones)


def test_origin_is_the_faced_offset(cases):
    d, n, _, pos, rays, flipped = cases
    faced = np.where(flipped[:, None], -n, n).astype(np.float64)
    want = r32(pos.astype(np.float64) + r32(faced * np.float64(F(0.01))))
    np.testing.assert_array_equal(bits(rays["origin"]), bits(want.astype(F)))
    assert (rays["t_min"] == 0).all() and (rays["t_max"] == F(25.0)).all()


def test_untraced_records_get_the_placeholder(cases):
    d, n, _, pos, rays, flipped = cases
    traced = np.arange(d.shape[0]) % 3 != 0
    some, fl = R.reflection_rays(d, pos, n, traced, 25.0)
    assert (some[~traced] == R.PLACEHOLDER[0]).all() and not fl[~traced].any()
    np.testing.assert_array_equal(some[traced].view(np.uint8), rays[traced].view(np.uint8))
    np.testing.assert_array_equal(fl[traced], flipped[traced])
