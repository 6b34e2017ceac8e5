"""Shade data and surface resolves without a device: the library exports the four entry points and the calls reject a null context
and bad arguments before any device work; the host-side checks and row packing of mrt_upload_shade_data
(csrc/host/shade_data_test.cpp); the numpy restatement (messyerraytracer_amd/surface.py, what the GPU tests hold the kernel to byte for
byte) against values recorded from the reference's own TriangleNormals::interpolate and TriangleUV::interpolate
(tests/golden/surface_reference.npz), bit for bit; the material half of extract_surface against hand-written cases."""
import ctypes as C
import os
import subprocess

import numpy as np

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import surface as S
from messyerraytracer_amd import types as T

P = C.c_void_p(16)  # a pointer no call may dereference: every case below fails its checks first
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surface_reference.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_exports_sizes_and_constants():
    L = capi.load()
    for s in ("mrt_upload_shade_data", "mrt_clear_shade_data", "mrt_resolve_surfaces", "mrt_resolve_grid_surfaces"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert L.mrt_struct_size(capi.STRUCT_MATERIAL) == T.MATERIAL.itemsize == 48
    assert L.mrt_struct_size(capi.STRUCT_SURFACE64) == T.SURFACE64.itemsize == 64
    assert L.mrt_struct_size(capi.STRUCT_SHADE_DATA) == C.sizeof(capi.ShadeData) == 48
    assert L.mrt_struct_size(capi.STRUCT_SURFACE_OUT) == C.sizeof(capi.SurfaceOut) == 24
    assert (capi.STRUCT_MATERIAL, capi.STRUCT_SHADE_DATA, capi.STRUCT_SURFACE64) == (6, 7, 8)
    assert L.mrt_struct_size(5) == 0 and L.mrt_struct_size(10) == 0
    assert capi.SHADE_ARRAYS_ON_DEVICE == 1 and T.DEFAULT_MATERIAL == 0xFFFFFFFF
    assert [n for n in T.MATERIAL.names] == ["albedo", "metallic", "roughness", "specular", "emission", "emission_energy", "flags", "reserved"]
    assert [T.MATERIAL.fields[n][1] for n in T.MATERIAL.names] == [0, 12, 16, 20, 24, 36, 40, 44]
    assert [T.SURFACE64.fields[n][1] for n in T.SURFACE64.names] == [0, 12, 16, 28, 32, 44, 48, 56, 60]


def test_null_context_and_bad_arguments_are_invalid():
    """(With a context, every bad argument is checked before any device work: test_surface_gpu.py.)"""
    L = capi.load()
    out = capi.SurfaceOut(16, 16, 16)
    none = capi.SurfaceOut(None, None, None)
    cam = capi.Camera()
    good = capi.ShadeData(C.sizeof(capi.ShadeData), 0, 0, 0, None, None, None, None)
    assert L.mrt_upload_shade_data(None, C.byref(good)) == capi.ERR_INVALID
    assert L.mrt_upload_shade_data(None, None) == capi.ERR_INVALID
    assert L.mrt_clear_shade_data(None) == capi.ERR_INVALID
    for o in (out, none, None):
        ref = None if o is None else C.byref(o)
        assert L.mrt_resolve_surfaces(None, P, P, 1, ref, 0) == capi.ERR_INVALID
        assert L.mrt_resolve_surfaces(None, P, P, 0, ref, 0) == capi.ERR_INVALID
        assert L.mrt_resolve_grid_surfaces(None, C.byref(cam), 4, 4, 0, 4, P, ref, 0) == capi.ERR_INVALID
    assert L.mrt_resolve_surfaces(None, None, P, 1, C.byref(out), 0) == capi.ERR_INVALID
    assert L.mrt_resolve_surfaces(None, P, None, 1, C.byref(out), 0) == capi.ERR_INVALID
    assert L.mrt_resolve_surfaces(None, P, P, 1, C.byref(out), 1 << 20) == capi.ERR_INVALID
    assert L.mrt_resolve_grid_surfaces(None, C.byref(cam), 4, 4, 3, 2, P, C.byref(out), 0) == capi.ERR_INVALID
    assert L.mrt_resolve_grid_surfaces(None, None, 4, 4, 0, 4, P, C.byref(out), 0) == capi.ERR_INVALID
    assert L.mrt_resolve_grid_surfaces(None, C.byref(cam), 4, 4, 0, 4, None, C.byref(out), 0) == capi.ERR_INVALID


def test_shade_data_driver():
    exe = mbuild.build_shade_data_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


# ---- the interpolations against the reference's own ---------------------------------------------------------------------------------

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        g = np.load(GOLDEN)
        _FIXTURE.append({k: g[k] for k in g.files})
    return _FIXTURE[0]


def test_fixture_covers_what_it_must():
    g = fixture()
    n9, u, v, kind = g["normals9"], g["u"], g["v"], g["kind"]
    assert 1900 <= u.shape[0] <= 2200 and n9.shape == (u.shape[0], 3, 3) and g["uvs6"].shape == (u.shape[0], 3, 2)
    assert (kind == 0).sum() >= 1000                                                                  # general
    w = (F(1) - u) - v
    assert ((w == 0) & (u > 0) & (v > 0)).sum() >= 60 and (w < 0).sum() >= 60                         # u + v at 1 and beyond
    one_ulp = np.abs(w[(kind == 2) | (kind == 3)])
    assert one_ulp.size >= 120 and (one_ulp > 0).all() and (one_ulp <= F(2.0 ** -23)).all()          # one ulp to either side
    assert ((kind == 2) & (w > 0)).sum() >= 60 and ((kind == 3) & (w < 0)).sum() >= 60
    assert ((u == 0) & (v != 0)).sum() >= 90 and ((v == 0) & (u != 0)).sum() >= 90 and ((u == 0) & (v == 0)).sum() >= 30
    zero = (g["normal"] == 0).all(axis=1)
    assert (zero & (kind == 7)).sum() >= 150 and ((n9[kind == 7] != 0).any(axis=(1, 2))).sum() >= 100   # cancelling, not all-zero inputs
    length = np.linalg.norm(n9.astype(np.float64), axis=2)
    assert ((length > 1.5) & np.isfinite(length)).any() and ((length < 0.5) & (length > 1e-4)).any()  # non-unit
    l2 = (length ** 2).min(axis=1)
    assert ((l2 < 1.1754944e-38) & (l2 > 0) & ~zero).sum() >= 40                                      # squared length denormal, result not zero
    assert ((kind == 9) & zero).sum() >= 20                                                           # ... or underflowing to zero
    assert np.isfinite(g["normal"]).all() and np.isfinite(g["uv"]).all()


def test_smooth_normal_equals_the_reference_bit_for_bit():
    g = fixture()
    n9 = g["normals9"]
    got = S.smooth_normal(n9[:, 0], n9[:, 1], n9[:, 2], g["u"], g["v"])
    np.testing.assert_array_equal(bits(got), bits(g["normal"]))


def test_interpolate_uv_equals_the_reference_bit_for_bit():
    g = fixture()
    uv = g["uvs6"]
    got = S.interpolate_uv(uv[:, 0], uv[:, 1], uv[:, 2], g["u"], g["v"])
    np.testing.assert_array_equal(bits(got), bits(g["uv"]))


def test_resolve_uses_both_interpolations():
    """resolve() on the fixture's tuples as one triangle each: the rows' normal and uv are the recorded ones."""
    g = fixture()
    n = g["u"].shape[0]
    shade = S.ShadeData(n, normals9=g["normals9"], uvs6=g["uvs6"])
    d = np.tile(np.array([0, 0, -1], F), (n, 1))
    rows, pairs, out_n = S.resolve(d, np.tile(np.array([0, 0, 1], F), (n, 1)), np.ones(n, bool), np.arange(n), g["u"], g["v"], shade)
    np.testing.assert_array_equal(bits(rows["normal"]), bits(g["normal"]))
    np.testing.assert_array_equal(bits(out_n), bits(g["normal"]))
    np.testing.assert_array_equal(bits(rows["uv"]), bits(g["uv"]))
    ndv = g["normal"][:, 2]   # vd = (0, 0, 1): (nx*0 + ny*0) + nz*1
    np.testing.assert_array_equal(bits(rows["n_dot_v"]), bits(np.where(ndv < F(0.001), F(0.001), ndv)))
    assert (rows["material"] == T.DEFAULT_MATERIAL).all() and (pairs == np.array([0, 0.5], F)).all()


# ---- the material half of extract_surface (shade_pass.h:535-573) against hand-written cases --------------------------------------

def materials():
    m = np.zeros(3, T.MATERIAL)
    m[0] = ((0.1, 0.2, 0.3), 0.25, 0.6, 0.7, (1.0, 2.0, 3.0), 0.0, 1, 0)       # energy 0 with an emission colour
    m[1] = ((0.9, 0.8, 0.7), 1.0, 0.02, 0.5, (0.5, 0.25, 2.0), 4.0, 2, 0)      # roughness below the clamp, an emitter
    m[2] = ((0.4, 0.4, 0.4), 0.0, 0.04, 0.0, (1.0, 1.0, 1.0), -1.0, 0, 0)      # roughness at the clamp, negative energy
    return m


def row(albedo, metallic, emission, roughness, specular, material):
    r = np.zeros(1, T.SURFACE64)
    r["albedo"], r["metallic"], r["emission"], r["roughness"], r["specular"], r["material"] = albedo, metallic, emission, roughness, specular, material
    return r[0]


DEFAULT_ROW = row((0.75, 0.75, 0.75), 0.0, (0, 0, 0), 0.5, 0.5, 0xFFFFFFFF)


def test_material_half_hand_written_cases():
    ids = np.array([0, 1, 2, 3, 0xFFFFFFFF], np.uint32)   # triangle 3: id == n_materials, triangle 4: far out of range
    shade = S.ShadeData(5, materials(), material_ids=ids)
    prim = np.array([0, 1, 2, 3, 4, 5, 0xFFFFFFFF, 0x80000000], np.uint32)   # 5 and up: prim id out of range
    got = S.material_surface(prim, shade)
    want = np.zeros(8, T.SURFACE64)
    want[0] = row((0.1, 0.2, 0.3), 0.25, (0, 0, 0), 0.6, 0.7, 0)                                  # energy 0: no emission
    want[1] = row((0.9, 0.8, 0.7), 1.0, (F(0.5) * F(4), F(0.25) * F(4), F(2) * F(4)), 0.04, 0.5, 1)   # 0.02 -> 0.04; energy > 0
    want[2] = row((0.4, 0.4, 0.4), 0.0, (0, 0, 0), 0.04, 0.0, 2)                                  # energy < 0: no emission
    want[3:] = DEFAULT_ROW                                                                        # id out of range, prim out of range
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_material_half_without_ids_materials_or_shade_data():
    prim = np.array([0, 1], np.uint32)
    for shade in (None, S.ShadeData(0), S.ShadeData(2, materials()), S.ShadeData(2, None, material_ids=np.zeros(2, np.uint32)),
                  S.ShadeData(0, materials(), material_ids=np.zeros(0, np.uint32))):
        got = S.material_surface(prim, shade)
        np.testing.assert_array_equal(got.view(np.uint32), np.array([DEFAULT_ROW, DEFAULT_ROW]).view(np.uint32))


def test_resolve_misses_and_defaults():
    d = np.array([[0, 0, -2], [0, 3, 0], [1, 0, 0]], F)
    nrm = np.array([[0, 0, 1], [0, 1, 0], [5, 6, 7]], F)
    hit = np.array([True, True, False])
    rows, pairs, out_n = S.resolve(d, nrm, hit, np.array([0, 7, 0xFFFFFFFF], np.uint32), np.zeros(3, F), np.zeros(3, F), None)
    assert rows["n_dot_v"][0] == 1 and rows["n_dot_v"][1] == F(0.001)          # facing the viewer; facing away: the floor
    np.testing.assert_array_equal(rows[:2]["normal"], nrm[:2])
    miss = np.zeros(1, T.SURFACE64)
    miss["material"] = 0xFFFFFFFF
    np.testing.assert_array_equal(rows[2:].view(np.uint32), miss.view(np.uint32))
    np.testing.assert_array_equal(pairs, np.array([[0, 0.5]] * 3, F))
    np.testing.assert_array_equal(out_n, nrm)                                 # a miss keeps whatever its record holds
