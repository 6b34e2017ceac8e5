"""Bounce casts without a device: the library exports mrt_cast_bounce / mrt_cast_grid_bounce and the calls reject a null context and
bad arguments before any device work; the launch policy plans them as reflection casts that never touch the primary grid's state
(csrc/host/record_policy_test.cpp); the numpy restatement of the sampler (messyerraytracer_amd/bounce.py, what the GPU tests hold the
kernels to byte for byte) against values recorded from the reference's own sample_bounce, ggx_sample_half and PCG32
(tests/golden/bounce_reference.npz); the diffuse lobe against hemisphere.py; the jump constants."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from messyerraytracer_amd import bounce as B
from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import hemisphere as H

P = C.c_void_p(16)  # a pointer no call may dereference: every case below fails its checks first
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bounce_reference.npz")
# the largest component differences between the restated half vector / direction and the reference's on the fixture, as measured
# (DESIGN §4.13): they differ only through the sincos pair.  Asserted with the 2x margin §4.12 uses for the same cause.
MEASURED_HALF_DIFF = 3.576279e-07
MEASURED_DIRECTION_DIFF = 5.383044e-07
NEAR_ZERO = 2 * MEASURED_DIRECTION_DIFF   # |n . dir| within this: the sign ("below surface") is rounding noise, a list of its own


def desc(frame=0, first_draw=0, t_max=1.0, metallic=0.5, roughness=0.5, surface=None):
    return capi.Bounce(frame, first_draw, t_max, metallic, roughness, None, surface, None)


def array_form(L, ctx=None, d=None, rays=P, hits=P, out=P, flags=0):
    d = desc() if d is None else d
    return L.mrt_cast_bounce(ctx, rays, hits, 1, C.byref(d) if d is not False else None, out, None, 0xFFFFFFFF, flags)


def grid_form(L, ctx=None, d=None, y0=0, y1=4, hits=P, out=P):
    d = desc() if d is None else d
    cam = capi.Camera()
    return L.mrt_cast_grid_bounce(ctx, C.byref(cam), 4, 4, y0, y1, hits, C.byref(d) if d is not False else None, out, None, 0xFFFFFFFF, 0)


def test_exports():
    L = capi.load()
    for s in ("mrt_cast_bounce", "mrt_cast_grid_bounce"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert C.sizeof(capi.Bounce) == 48
    assert (capi.LOBE_NONE, capi.LOBE_DIFFUSE, capi.LOBE_SPECULAR) == (B.LOBE_NONE, B.LOBE_DIFFUSE, B.LOBE_SPECULAR) == (0, 1, 2)


def test_null_context_and_bad_arguments_are_invalid():
    """(With a context, every bad argument is checked before the scene and before any device work: test_bounce_gpu.py.)"""
    L = capi.load()
    assert array_form(L) == capi.ERR_INVALID and grid_form(L) == capi.ERR_INVALID
    for form in (array_form, grid_form):
        for t in (math.nan, math.inf, -math.inf, 1e-4, 0.0, -1.0):
            assert form(L, d=desc(t_max=t)) == capi.ERR_INVALID
        for x in (math.nan, math.inf, -math.inf, -0.01, 1.01):
            assert form(L, d=desc(metallic=x)) == capi.ERR_INVALID
            assert form(L, d=desc(roughness=x)) == capi.ERR_INVALID
        assert form(L, d=False) == capi.ERR_INVALID
        assert form(L, hits=None) == capi.ERR_INVALID and form(L, out=None) == capi.ERR_INVALID
    assert array_form(L, rays=None) == capi.ERR_INVALID and array_form(L, flags=1 << 20) == capi.ERR_INVALID
    assert grid_form(L, y0=3, y1=2) == capi.ERR_INVALID


def test_bounce_policy_driver():
    exe = mbuild.build_record_policy_test()
    r = subprocess.run([exe, "bounce"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


class Fixture:
    def __init__(self):
        g = np.load(GOLDEN)
        self.g = g
        self.seeds, self.fd, self.n, self.v = g["seeds"], g["first_draws"], g["normals"], g["views"]
        self.count = self.seeds.shape[0]
        self.du = np.zeros((self.count, 3), np.uint32)
        for f in np.unique(self.fd):
            k = self.fd == f
            for j in range(3):
                self.du[k, j] = B.draw(self.seeds[k], int(f) + j)
        self.u = H.to_float(self.du)
        self.m, self.ro = B.clamp_surface(g["metallic"], g["roughness"])
        # (the incoming direction of a view direction v is -v: exact)
        self.dirs, self.spec, self.sp, _ = B.bounce_direction(self.n, -self.v, self.m, self.ro, self.u[:, 0], self.u[:, 1], self.u[:, 2])
        self.h, self.cos, self.sin = B.ggx_half(self.n, self.ro, self.u[:, 1], self.u[:, 2])


_FIXTURE = []


def fixture():
    if not _FIXTURE:
        _FIXTURE.append(Fixture())
    return _FIXTURE[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_fixture_covers_what_it_must():
    fx = fixture()
    g, u, n = fx.g, fx.g["draws_f32"], fx.n
    assert 1900 <= fx.count <= 2200
    assert (g["lobe"] == 1).sum() > 400 and (g["lobe"] == 2).sum() > 400 and set(np.unique(g["lobe"])) == {1, 2}
    ro_in = g["roughness"]
    for r in (0.04, 0.3, 1.0):
        assert (ro_in == F(r)).sum() > 50
    assert (ro_in < F(0.04)).sum() > 50 and (fx.ro >= F(0.04)).all()                        # below the clamp
    assert (g["spec_prob"] == F(0.05)).sum() > 30 and (g["spec_prob"] == F(0.95)).sum() > 30      # both clamps of sp
    u0, sp = u[:, 0], g["spec_prob"]
    assert (u0 == sp).sum() >= 90 and (np.nextafter(u0, F(1)) == sp).sum() >= 90 and (np.nextafter(u0, F(0)) == sp).sum() >= 90
    assert (u[:, 1] == 0).sum() >= 16 and (u[:, 1] == 1).sum() >= 32
    for lobe in (1, 2):
        assert ((u[:, 1] == 0) & (g["lobe"] == lobe)).any() and ((u[:, 1] == 1) & (g["lobe"] == lobe)).any()
    vn = fx.v.astype(np.float64) / np.linalg.norm(fx.v.astype(np.float64), axis=1)[:, None]
    ndv = (n.astype(np.float64) * vn).sum(axis=1)
    assert ((ndv > 2e-4) & (ndv < 3e-3)).sum() > 150                                       # grazing views
    assert (n[:, 2] < -0.999).sum() > 100 and (np.abs(n[:, 2]) < 1e-2).sum() > 100
    assert ((n[:, 2] == 0) & np.signbit(n[:, 2])).any() and ((n[:, 2] == 0) & ~np.signbit(n[:, 2])).any()
    assert (g["valid"] == 0).sum() > 50 and (g["valid"] == 1).sum() > 1000


def test_draws_spec_prob_lobe_and_angles_equal_the_reference_exactly():
    fx = fixture()
    g = fx.g
    np.testing.assert_array_equal(fx.du, g["draws_u32"])
    np.testing.assert_array_equal(bits(fx.u), bits(g["draws_f32"]))
    np.testing.assert_array_equal(bits(fx.sp), bits(g["spec_prob"]))
    np.testing.assert_array_equal(np.where(fx.spec, B.LOBE_SPECULAR, B.LOBE_DIFFUSE), g["lobe"])
    np.testing.assert_array_equal(bits(fx.cos), bits(g["cos_theta"]))
    np.testing.assert_array_equal(bits(fx.sin), bits(g["sin_theta"]))


def test_half_vector_and_direction_against_the_reference():
    fx = fixture()
    g = fx.g
    assert np.isfinite(fx.h).all() and np.isfinite(fx.dirs).all() and np.isfinite(g["directions"]).all()
    dh = float(np.abs(fx.h.astype(np.float64) - g["half"].astype(np.float64)).max())
    dd = float(np.abs(fx.dirs.astype(np.float64) - g["directions"].astype(np.float64)).max())
    print("largest component difference to the reference: half vector %.6e (bound %.6e), direction %.6e (bound %.6e)"
          % (dh, 2 * MEASURED_HALF_DIFF, dd, 2 * MEASURED_DIRECTION_DIFF))
    assert dh <= 2 * MEASURED_HALF_DIFF and dd <= 2 * MEASURED_DIRECTION_DIFF


def test_validity_agrees_with_the_reference_away_from_zero():
    """n . dir decides "below surface".  Where the reference's own |n . dir| exceeds the direction bound the restatement must decide as
    the reference did.  The tuples inside the bound (u1 == 1 in the diffuse lobe: the direction lies in the tangent plane) are a list
    of their own, at most 2 % of the fixture: there both sides hold |n . dir| to the bound and the sign is not compared."""
    fx = fixture()
    g, n, d = fx.g, fx.n, fx.dirs
    nd = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    near = np.abs(g["n_dot_dir"]) <= F(NEAR_ZERO)
    print("%d of %d tuples have |n . dir| <= %.3e in the reference" % (near.sum(), fx.count, NEAR_ZERO))
    assert 0 < near.sum() <= 0.02 * fx.count
    np.testing.assert_array_equal(~(nd[~near] <= 0), g["valid"][~near].astype(bool))
    np.testing.assert_array_equal(~(g["n_dot_dir"][~near] <= 0), g["valid"][~near].astype(bool))
    print("on that list: |n . dir| restated <= %.3e, reference <= %.3e" % (np.abs(nd[near]).max(), np.abs(g["n_dot_dir"][near]).max()))
    assert float(np.abs(nd[near]).max()) <= NEAR_ZERO and float(np.abs(g["n_dot_dir"][near]).max()) <= NEAR_ZERO


def test_diffuse_lobe_is_the_hemisphere_sample_one_draw_later():
    fx = fixture()
    diffuse = ~fx.spec
    assert diffuse.sum() > 400
    for f in np.unique(fx.fd):
        k = diffuse & (fx.fd == f)
        want, _, _ = H.sample_direction(fx.seeds[k], fx.n[k], first_draw=int(f) + 1)
        np.testing.assert_array_equal(bits(fx.dirs[k]), bits(want))


def test_a_jump_reaches_the_draws_a_stepping_generator_reaches():
    """first_draw 0, 1, 3, 6, 10 against hemisphere.py's stepping generator, and all of them and 2^31 + 5 against draws the
    reference's own generator reached by stepping."""
    g = np.load(GOLDEN)
    seeds = g["seeds"][:256]
    stepped = H.draws(seeds, 13)
    for k in (0, 1, 3, 6, 10):
        assert B.jump(k) == H.jump(k)
        for j in range(3):
            np.testing.assert_array_equal(B.draw(seeds, k + j), stepped[:, k + j], err_msg="draw %d" % (k + j))
    js, jf, jd = g["jump_seeds"], g["jump_first_draws"], g["jump_draws_u32"]
    assert set(int(x) for x in jf) == {0, 1, 3, 6, 10, (1 << 31) + 5}
    for i in range(js.shape[0]):
        got = [int(B.draw(js[i:i + 1], int(jf[i]) + j)[0]) for j in range(3)]
        assert got == [int(x) for x in jd[i]], (int(js[i]), int(jf[i]))


def test_material_clamps():
    m, ro = B.clamp_surface(np.array([-1, 0, 0.5, 1, 2, np.nan], F), np.array([-1, 0.02, 0.04, 1, 2, np.nan], F))
    np.testing.assert_array_equal(m, np.array([0, 0, 0.5, 1, 1, 0], F))
    np.testing.assert_array_equal(ro, np.array([0.04, 0.04, 0.04, 1, 1, 0.04], F))
    sp = B.spec_prob(np.array([0, 1, 0, 0.5], F), np.array([1, 0.3, 0.04, 0.3], F))
    np.testing.assert_array_equal(sp, np.array([0.05, 0.95, F(0.96) * F(0.5), F(0.5) + (F(0.5) * F(0.7)) * F(0.5)], F))
