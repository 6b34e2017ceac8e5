"""Hemisphere casts without a device: the library exports mrt_cast_hemisphere / mrt_cast_grid_hemisphere and the calls reject a null
context and bad arguments before any device work; the launch policy plans them as unsorted non-coherent batches that never touch the
primary grid's state (csrc/host/record_policy_test.cpp); the numpy restatement of the sampler (messyerraytracer_amd/hemisphere.py,
what the GPU tests hold the kernels to byte for byte) against values recorded from the reference's own PCG32 and
cosine_hemisphere_sample (tests/golden/hemisphere_reference.npz), and the accuracy condition on its sincos pair."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import hemisphere as H

P = C.c_void_p(16)  # a pointer no call may dereference: every case below fails its checks first
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hemisphere_reference.npz")
# the largest component difference between the restated direction and the reference's on the fixture, as measured:
# the two differ only through the sincos pair
MEASURED_DIRECTION_DIFF = 3.874302e-07


def desc(n_samples=4, frame=0, first_draw=1, t_max=1.0):
    return capi.Hemisphere(n_samples, frame, first_draw, t_max, None)


def array_form(L, ctx=None, d=None, out_rays=None, mode=capi.MODE_ANY_HIT, rays=P, hits=P, out=P, flags=0):
    d = desc() if d is None else d
    return L.mrt_cast_hemisphere(ctx, rays, hits, 1, C.byref(d) if d is not False else None, out, out_rays, 0xFFFFFFFF, mode, flags)


def grid_form(L, ctx=None, d=None, out_rays=None, mode=capi.MODE_ANY_HIT, y0=0, y1=4, hits=P, out=P):
    d = desc() if d is None else d
    cam = capi.Camera()
    return L.mrt_cast_grid_hemisphere(ctx, C.byref(cam), 4, 4, y0, y1, hits, C.byref(d) if d is not False else None, out, out_rays,
                                      0xFFFFFFFF, mode, 0)


def test_exports():
    L = capi.load()
    for s in ("mrt_cast_hemisphere", "mrt_cast_grid_hemisphere"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert C.sizeof(capi.Hemisphere) == 24


def test_null_context_and_bad_arguments_are_invalid():
    """(With a context, every bad argument is checked before the scene and before any device work: test_hemisphere_gpu.py.)"""
    L = capi.load()
    assert array_form(L) == capi.ERR_INVALID and grid_form(L) == capi.ERR_INVALID
    for form in (array_form, grid_form):
        for n in (0, 17):
            assert form(L, d=desc(n_samples=n)) == capi.ERR_INVALID
        for t in (math.nan, math.inf, -math.inf, 1e-4, 0.0, -1.0):
            assert form(L, d=desc(t_max=t)) == capi.ERR_INVALID
        assert form(L, out_rays=P, mode=capi.MODE_ANY_HIT) == capi.ERR_INVALID
        assert form(L, d=False) == capi.ERR_INVALID
        assert form(L, mode=2) == capi.ERR_INVALID
    assert grid_form(L, y0=3, y1=2) == capi.ERR_INVALID


def test_hemisphere_policy_driver():
    exe = mbuild.build_record_policy_test()
    r = subprocess.run([exe, "hemisphere"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


def test_pcg32_equals_the_reference():
    g = np.load(GOLDEN)
    seeds, du, df = g["seeds"], g["draws_u32"], g["draws_f32"]
    assert seeds.shape[0] >= 2000 and du.shape == (seeds.shape[0], 8)
    got = H.draws(seeds, 8)
    np.testing.assert_array_equal(got, du)
    np.testing.assert_array_equal(H.to_float(got).view(np.uint32), df.view(np.uint32))
    ones = df == F(1.0)
    assert ones[:, 1].any() and ones[:, 2:].any() and not ones[:, 0].any()  # next_float does return 1.0 (as u1: the edge list below)
    assert (du[ones] >= 0xFFFFFF80).all() and (df <= F(1.0)).all() and (df >= 0).all()
    edge = H.draws(g["edge_seeds"], 8)
    np.testing.assert_array_equal(edge, g["edge_draws_u32"])
    np.testing.assert_array_equal(H.to_float(edge).view(np.uint32), g["edge_draws_f32"].view(np.uint32))
    assert (g["edge_draws_f32"][:, 0] == F(1.0)).all()


def test_jump_constants_reach_every_draw():
    g = np.load(GOLDEN)
    seeds = g["seeds"][:256]
    stepped = H.draws(seeds, 34)
    for k in range(34):
        np.testing.assert_array_equal(H.draw(seeds, k), stepped[:, k], err_msg="draw %d" % k)
    assert H.jump(0) == (1, 0) and H.jump(1) == (H.MUL, H.INC)
    np.testing.assert_array_equal(stepped[:, :8], g["draws_u32"][:256])


def test_direction_against_the_reference():
    g = np.load(GOLDEN)
    seeds, n, want = g["seeds"], g["normals"], g["directions"]
    assert (n[:, 2] < -0.999).sum() > 100 and (np.abs(n[:, 2]) < 1e-2).sum() > 100      # z near -1, and z on both sides of 0
    assert np.signbit(n[:, 2]).any() and (~np.signbit(n[:, 2])).any() and (n[:, 2] == 0).any()
    got, u1, u2 = H.sample_direction(seeds, n)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print("largest component difference to the reference's direction: %.6e (bound %.6e)" % (diff, 2 * MEASURED_DIRECTION_DIFF))
    assert diff <= 2 * MEASURED_DIRECTION_DIFF
    length = np.sqrt((got.astype(np.float64) ** 2).sum(axis=1))
    worst = float(np.abs(length - 1.0).max())
    print("largest | |dir| - 1 |: %.3e (2 ulp of 1: %.3e)" % (worst, 2 * 2.0 ** -23))
    assert worst <= 2 * 2.0 ** -23
    dot = lambda d: (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]  # noqa: E731  (float32, the kernel's expression)
    ref_above = dot(want) >= 0
    assert ref_above.sum() > 2000 - 16
    assert (dot(got)[ref_above] >= 0).all()
    assert ref_above.all() and (u1 < F(1.0)).all()     # (every sample of this list is a valid one in the reference)


def test_direction_in_the_tangent_plane_when_u1_is_one():
    """The fixture's edge list: seeds whose first draw is exactly 1.0, so z = sqrt(max(0, 1 - u1)) = 0 and the direction lies in the
    tangent plane.  n . dir is then rounding noise around 0 on both sides -- the reference's own values on this list lie between
    -9.1e-8 and 1.2e-7, 14 of the 32 exactly 0 -- and its sign decides "below surface" (no ray).  So the sign is not compared here;
    the direction is, with the bound of the main list, and |n . dir| is held to 8 * 2^-24: the basis, the sum, the normalisation
    and the dot product are about eight roundings of 2^-24 each on values of at most 1."""
    g = np.load(GOLDEN)
    seeds, n, want = g["edge_seeds"], g["edge_normals"], g["edge_directions"]
    assert seeds.shape[0] == 32
    got, u1, _ = H.sample_direction(seeds, n)
    assert (u1 == F(1.0)).all()
    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print("u1 == 1: largest component difference to the reference's direction: %.6e" % diff)
    assert diff <= 2 * MEASURED_DIRECTION_DIFF
    assert float(np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max()) <= 2 * 2.0 ** -23
    for name, d in (("restated", got), ("reference", want)):
        dt = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        print("u1 == 1: n . dir of the %s directions in [%.3e, %.3e]" % (name, dt.min(), dt.max()))
        assert float(np.abs(dt).max()) <= 8 * 2.0 ** -24
    dt = (n[:, 0] * got[:, 0] + n[:, 1] * got[:, 1]) + n[:, 2] * got[:, 2]
    assert (dt > 0).any() and (dt <= 0).any()   # both outcomes occur: some of these entries get a ray, some do not


def sincos_inputs():
    rng = np.random.default_rng(1)
    yield (np.arange(0, 1 << 24, dtype=np.float64) / (1 << 24)).astype(F)       # every j * 2^-24
    yield H.to_float(rng.integers(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(np.uint32))  # 2^22 draws as next_float scales them
    yield np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0], dtype=F)      # the quadrant boundaries, ties of rint


def test_sincos_pair_is_no_farther_from_the_truth_than_the_reference_formula():
    """On every u2 = j * 2^-24 and 2^22 random draws: the restated pair is nowhere farther from float64 cos / sin(2 pi u2) than the
    reference's float32 formula is at its worst.  The reference's side is taken at its best: phi = 2 * PT_PI * u2 rounded as float32
    does, then a correctly rounded float32 cos / sin of that phi (no math library's float32 error added), so the bound is the tighter
    one."""
    ours_c = ours_s = ref_c = ref_s = 0.0
    for u in sincos_inputs():
        for lo in range(0, u.shape[0], 1 << 22):
            v = u[lo:lo + (1 << 22)]
            c, s = H.sincos_2pi(v)
            t = 2.0 * np.pi * v.astype(np.float64)
            tc, ts = np.cos(t), np.sin(t)
            ours_c = max(ours_c, float(np.abs(c - tc).max()))
            ours_s = max(ours_s, float(np.abs(s - ts).max()))
            phi = (F(2.0) * F(3.14159265358979323846) * v).astype(np.float64)
            ref_c = max(ref_c, float(np.abs(np.cos(phi).astype(F) - tc).max()))
            ref_s = max(ref_s, float(np.abs(np.sin(phi).astype(F) - ts).max()))
    print("largest error  ours: cos %.3e sin %.3e   the reference's formula: cos %.3e sin %.3e" % (ours_c, ours_s, ref_c, ref_s))
    assert ours_c <= ref_c and ours_s <= ref_s
    assert ours_c <= 1e-7 and ours_s <= 1e-7         # what include/mrt_hip.h states about the pair
    c, s = H.sincos_2pi(np.array([0.0, 0.25, 0.5, 0.75, 1.0], dtype=F))                   # exact on the axes
    np.testing.assert_array_equal(c, np.array([1, 0, -1, 0, 1], dtype=F))
    np.testing.assert_array_equal(s, np.array([0, 1, 0, -1, 0], dtype=F))
