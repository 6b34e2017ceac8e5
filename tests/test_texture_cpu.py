"""Resident textures and the textured resolve without a device: the library exports the two entry points, the struct sizes and layouts
agree and the calls reject a null context; the host-side refusals and the pool's layout (csrc/host/texture_data_test.cpp); the numpy
restatement (messyerraytracer_amd/texture.py, what the GPU tests hold the kernel to byte for byte) against values recorded from the
reference's own TextureSampler::sample_bilinear (texture_sampler.h:45-88), TriangleTangents (triangle_tangents.h:21-56), perturb_normal
(shade_pass.h:110-162) and extract_surface (shade_pass.h:509-587) in tests/golden/texture_reference.npz.  Only floorf,
sqrtf and fp32 arithmetic enter, so every tuple is compared bit for bit: no tolerance, no tuple left out."""
import ctypes as C
import os
import subprocess

import numpy as np

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import surface as S
from messyerraytracer_amd import texture as X
from messyerraytracer_amd import types as T

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_reference.npz")
N_IMAGES = 14

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        g = np.load(GOLDEN)
        g = {k: g[k] for k in g.files}
        g["images"] = [g[f"image_{k}"] for k in range(N_IMAGES)]
        _FIXTURE.append(g)
    return _FIXTURE[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_exports_sizes_and_layouts():
    L = capi.load()
    for s in ("mrt_upload_textures", "mrt_clear_textures"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert (capi.STRUCT_TEXTURE, capi.STRUCT_MATERIAL_TEXTURES, capi.STRUCT_TEXTURE_SET) == (18, 19, 20)
    assert L.mrt_struct_size(capi.STRUCT_TEXTURE) == C.sizeof(capi.Texture) == 24
    assert L.mrt_struct_size(capi.STRUCT_MATERIAL_TEXTURES) == T.MATERIAL_TEXTURES.itemsize == 16
    assert L.mrt_struct_size(capi.STRUCT_TEXTURE_SET) == C.sizeof(capi.TextureSet) == 48
    assert L.mrt_struct_size(17) == 0 and L.mrt_struct_size(21) == 0
    assert [getattr(capi.Texture, n).offset for n, _ in capi.Texture._fields_] == [0, 4, 8, 12, 16]
    assert [getattr(capi.TextureSet, n).offset for n, _ in capi.TextureSet._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 40]
    assert [T.MATERIAL_TEXTURES.fields[n][1] for n in T.MATERIAL_TEXTURES.names] == [0, 4, 8, 12]
    # mrt_material and mrt_shade_data are as they were
    assert L.mrt_struct_size(capi.STRUCT_MATERIAL) == 48 and L.mrt_struct_size(capi.STRUCT_SHADE_DATA) == C.sizeof(capi.ShadeData)
    assert (X.NO_TEXTURE, T.NO_TEXTURE, T.TEXTURE_MAX_DIM) == (0xFFFFFFFF, 0xFFFFFFFF, 16384)


def test_null_context_is_invalid():
    """(With a context, every bad descriptor is refused before any device work: test_texture_gpu.py.)"""
    L = capi.load()
    d = capi.TextureSet(C.sizeof(capi.TextureSet), 0, 0, 0, 0, 0, None, None, None)
    assert L.mrt_upload_textures(None, C.byref(d)) == capi.ERR_INVALID and L.mrt_upload_textures(None, None) == capi.ERR_INVALID
    assert L.mrt_clear_textures(None) == capi.ERR_INVALID


def test_texture_data_driver():
    exe = mbuild.build_texture_data_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


def test_fixture_covers_what_it_must():
    g = fixture()
    sizes = [(im.shape[1], im.shape[0], im.dtype) for im in g["images"][:10]]
    assert sizes == [(w, h, dt) for dt in (np.uint8, np.float32) for (w, h) in ((1, 1), (2, 2), (3, 5), (8, 8), (64, 16))]
    img, uv, kind = g["s_img"], g["s_uv"], g["s_kind"]
    for k in range(10):
        m = img == k
        w, h = sizes[k][0], sizes[k][1]
        assert (m & (kind == 0)).sum() >= 64                                              # general, -3 .. 3
        a = uv[m]
        assert (a[kind[m] == 0].min() < -2) and (a[kind[m] == 0].max() > 2)
        for x in (0.0, 1.0, -1.0, 1e6, 1e30, -1e30, -1e-10, -0.25):
            assert (a[:, 0] == F(x)).any() and (a[:, 1] == F(x)).any(), (k, x)
        for x in (1.0, 2.0, -1.0, 0.0):                                                   # one ulp below an integer
            assert (a[:, 0] == np.nextafter(F(x), F(-np.inf))).any(), (k, x)
        assert ((a[:, 0] < 0) & ((a[:, 0] - np.floor(a[:, 0])).astype(F) == 1)).any()    # tiny negative: u - floor(u) rounds to 1
        assert (a[:, 0] == F(0.5 / w)).any() and (a[:, 1] == F(0.5 / h)).any()           # a texel centre
        assert (kind[m] == 1).sum() >= 1 and (kind[m] == 2).sum() >= 2
    pk, pin = g["p_kind"], g["p_in"]
    for k, least in ((0, 500), (1, 64), (2, 100), (3, 64), (4, 64), (5, 64), (6, 32), (7, 32)):
        assert (pk == k).sum() >= least, k
    scale = pin[:, 24]
    for x in (0.0, 1.0, 4.0):
        assert (scale == F(x)).sum() >= 100
    assert (pin[pk == 1][:, 13:16] == 0).all()                                            # zero signs
    assert (g["p_out"][pk == 1] == pin[pk == 1][:, 1:4]).all()                            # ... give the smooth normal back
    signs = pin[pk == 2][:, 13:16]
    assert ((signs > 0).any(axis=1) & (signs < 0).any(axis=1)).sum() >= 50                # mixed signs
    tan, _ = X.interpolate_tangent(pin[pk == 3][:, 4:16], pin[pk == 3][:, 16], pin[pk == 3][:, 17])
    assert (tan == F([1, 0, 0])).all(axis=1).sum() >= 48                                  # degenerate sums fall back to (1, 0, 0)
    par = pin[pk == 4]
    assert ((par[:, 4:7] == par[:, 1:4]).all(axis=1) | (par[:, 4:7] == -par[:, 1:4]).all(axis=1)).sum() >= 32   # T = +-N exactly
    flat = pin.view(np.uint32)[:, 0]
    assert (flat[pk == 5] == 10).sum() >= 16 and (flat[pk == 5] == 11).sum() >= 16
    zero = (pk == 5) & (flat == 11)                                                       # the sample cancels: l2(P) < 1e-8
    assert (g["p_out"][zero] == pin[zero][:, 1:4]).all()
    near = (pk == 5) & (flat == 13) & (scale == 0)                                        # ts = (0, 0, 4e-5): l2(P) = 1.6e-9
    assert near.sum() >= 4 and (g["p_out"][near] == pin[near][:, 1:4]).all()
    ek = g["e_kind"]
    for k in range(4):                                                                    # neither, albedo, normal, both
        assert (ek == k).sum() >= 250
    fl = g["e_in"].view(np.uint32)[:, 8]
    assert ((fl & 16) == 0).sum() >= 100 and ((fl & 32) == 0).sum() >= 100 and ((fl & 63) == 63).sum() >= 240
    for bit in (1, 2, 4, 8):
        assert ((fl & bit) == 0).sum() >= 200


def test_sample_bilinear_equals_the_reference_bit_for_bit():
    g = fixture()
    got = X.sample_textures(g["images"], g["s_img"], g["s_uv"][:, 0], g["s_uv"][:, 1])
    np.testing.assert_array_equal(bits(got), bits(g["s_out"]))
    # by hand: a texel centre gives the texel; the middle of a 2 x 2 image's horizontal edge the mean of c00 and c10 along x
    im = g["images"][6]                                                                   # 2 x 2, float
    np.testing.assert_array_equal(X.sample_bilinear(im, F([0.25]), F([0.25]))[0], im[0, 0])
    np.testing.assert_array_equal(X.sample_bilinear(im, F([0.75]), F([0.25]))[0], im[0, 1])
    np.testing.assert_array_equal(X.sample_bilinear(im, F([0.5]), F([0.25]))[0], X.lerp(im[0, 0], im[0, 1], F(0.5)))
    one = g["images"][0]                                                                  # 1 x 1, bytes: every UV gives byte / 255
    np.testing.assert_array_equal(bits(X.sample_bilinear(one, F([0.3, -7.5, 1e30]), F([0.9, 0.0, -1.0]))), bits(np.tile(one[0, 0].astype(F) / F(255), (3, 1))))


def test_perturb_normal_equals_the_reference_bit_for_bit():
    g = fixture()
    pin = g["p_in"]
    words = pin.view(np.uint32)
    img, has_uv, has_tan = words[:, 0], words[:, 25] != 0, words[:, 26] != 0
    smooth, tan12, u, v, scale = pin[:, 1:4], pin[:, 4:16], pin[:, 16], pin[:, 17], pin[:, 24]
    uv = S.interpolate_uv(pin[:, 18:20], pin[:, 20:22], pin[:, 22:24], u, v)
    run = has_uv & has_tan & X.has_tangents(tan12)
    got = smooth.copy()
    sample = X.sample_textures(g["images"], img[run], uv[run, 0], uv[run, 1])
    got[run] = X.perturb_normal(smooth[run], tan12[run], u[run], v[run], sample, scale[run])
    np.testing.assert_array_equal(bits(got), bits(g["p_out"]))
    assert (bits(got[run]) != bits(smooth[run])).any(axis=1).sum() >= 700


def _extract_groups(g):
    """The extract_surface tuples as batches resolve_textured takes: one batch per set of resident arrays, tuple i as triangle i with its
    own material i and binding i; a prim out of range is n + i, an id out of range n + i."""
    ein = g["e_in"]
    words = ein.view(np.uint32)
    fl = words[:, 8]
    for present in np.unique(fl & 15):
        idx = np.nonzero((fl & 15) == present)[0]
        n = idx.shape[0]
        e, w = ein[idx], words[idx]
        mats = np.zeros(n, T.MATERIAL)
        mats["albedo"], mats["metallic"], mats["roughness"], mats["specular"] = e[:, 36:39], e[:, 39], e[:, 40], e[:, 41]
        mats["emission"], mats["emission_energy"] = e[:, 42:45], e[:, 45]
        ids = np.where((w[:, 8] & 32) != 0, np.arange(n), n + np.arange(n)).astype(np.uint32)
        prim = np.where((w[:, 8] & 16) != 0, np.arange(n), n + np.arange(n)).astype(np.uint32)
        shade = S.ShadeData(n, mats, ids if present & 2 else None, e[:, 9:18].reshape(n, 3, 3) if present & 1 else None,
                            e[:, 18:24].reshape(n, 3, 2) if present & 4 else None)
        b = np.zeros(n, T.MATERIAL_TEXTURES)
        b["albedo_texture"], b["normal_texture"], b["normal_scale"] = w[:, 46], w[:, 47], e[:, 48]
        tex = X.TextureSet(g["images"], b, e[:, 24:36] if present & 8 else None)
        yield idx, e, prim, shade, tex


def test_extract_surface_equals_the_reference_bit_for_bit():
    g = fixture()
    changed_n = changed_a = 0
    for idx, e, prim, shade, tex in _extract_groups(g):
        hit = np.ones(idx.shape[0], bool)
        rows, pairs, n = X.resolve_textured(e[:, 0:3], e[:, 3:6], hit, prim, e[:, 6], e[:, 7], shade, tex)
        want = g["e_out"][idx]
        np.testing.assert_array_equal(bits(rows["normal"]), bits(want[:, 0:3]))
        np.testing.assert_array_equal(bits(n), bits(want[:, 0:3]))
        np.testing.assert_array_equal(bits(rows["n_dot_v"]), bits(want[:, 3]))
        np.testing.assert_array_equal(bits(rows["albedo"]), bits(want[:, 4:7]))
        np.testing.assert_array_equal(bits(rows["metallic"]), bits(want[:, 7]))
        np.testing.assert_array_equal(bits(rows["roughness"]), bits(want[:, 8]))
        np.testing.assert_array_equal(bits(rows["specular"]), bits(want[:, 9]))
        np.testing.assert_array_equal(bits(rows["emission"]), bits(want[:, 10:13]))
        np.testing.assert_array_equal(bits(pairs), bits(want[:, 7:9]))
        plain, _, plain_n = S.resolve(e[:, 0:3], e[:, 3:6], hit, prim, e[:, 6], e[:, 7], shade)
        changed_n += int((bits(plain_n) != bits(n)).any(axis=1).sum())
        changed_a += int((bits(plain["albedo"]) != bits(rows["albedo"])).any(axis=1).sum())
    assert changed_n >= 200 and changed_a >= 300                                          # the textures did something


def test_resolve_textured_without_a_binding_is_the_plain_resolve():
    """Nothing resident, no bindings, bindings of MRT_NO_TEXTURE, ids absent, UVs absent and a UV that is not finite: S.resolve's rows."""
    g = fixture()
    idx, e, prim, shade, tex = next(x for x in _extract_groups(g) if x[3].uvs6 is not None and x[3].material_ids is not None and x[3].normals9 is not None and x[4].tangents12 is not None)
    n = idx.shape[0]
    hit = np.ones(n, bool)
    args = (e[:, 0:3], e[:, 3:6], hit, prim, e[:, 6], e[:, 7])
    plain = S.resolve(*args, shade)
    none = X.bindings([None] * n, [None] * n, np.ones(n, F))
    for t in (None, X.TextureSet(g["images"]), X.TextureSet(g["images"], none, tex.tangents12)):
        for a, b in zip(X.resolve_textured(*args, shade, t), plain):
            np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    for absent in (S.ShadeData(n, shade.materials, None, shade.normals9, shade.uvs6), S.ShadeData(n, shade.materials, shade.material_ids, shade.normals9, None)):
        for a, b in zip(X.resolve_textured(*args, absent, tex), S.resolve(*args, absent)):
            np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    uvs = shade.uvs6.copy()
    uvs[::3, 0, 0], uvs[1::3, 2, 1] = np.nan, np.inf                                      # two thirds of the records: a UV not finite
    bad = S.ShadeData(n, shade.materials, shade.material_ids, shade.normals9, uvs)
    got, want = X.resolve_textured(*args, bad, tex), S.resolve(*args, bad)
    k = ~np.isfinite(want[0]["uv"]).all(axis=1)
    assert k.sum() >= n // 2
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32))
    assert (got[0]["albedo"][~k] != want[0]["albedo"][~k]).any()
