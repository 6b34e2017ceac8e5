"""mrt_upload_textures / mrt_clear_textures and the two resolves with a texture set resident: albedo textures and normal maps sampled on
the device, held to the numpy float32 restatement (messyerraytracer_amd/texture.py; pinned to the reference by test_texture_cpu.py)
byte for byte -- the 64-byte rows as uint32 words, the bounce pairs, the records with the perturbed normal.  The scenes, grids and
shade data of test_surface_gpu.py with seeded UVs over -3 .. 3 (wraps occur) and seeded tangents; eight textures, 1 x 1, 2 x 2, 3 x 5
and 8 x 8 in both formats, the 1 x 1 ones between the larger ones in the pool, so that an index one texel off reads a neighbour's
texel and differs; bindings under which both textures, albedo only, normal only on a triangle without tangents, an id past
n_bindings and a prim past n_tangent_tris all occur among the hits of every grid."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import path as P
from messyerraytracer_amd import surface as S
from messyerraytracer_amd import texture as X
from oracle import pyoracle as po
from test_hemisphere_gpu import DEV, Dev, Run, hit_point, same, scene
from test_lighting_gpu import environment, light_list
from test_path_gpu import FRAME, Outputs
from test_surface_gpu import GRIDS, GRID_IDS, ID_PERIOD, KINDS, N_MATERIALS, shade_data, words

pytestmark = pytest.mark.gpu

F = np.float32
NONE = X.NO_TEXTURE
N_BINDINGS = 5                    # materials 5 and 6 have no binding
GUARD = 64

SHADE, TEXTURES = {}, {}


def textured_shade(kind):
    """test_surface_gpu's shade data with UVs over -3 .. 3"""
    if kind not in SHADE:
        s = shade_data(kind)
        rng = np.random.default_rng(4180 + len(kind))
        SHADE[kind] = S.ShadeData(s.n_tris, s.materials, s.material_ids, s.normals9, rng.uniform(-3, 3, size=(s.n_tris, 3, 2)).astype(F))
    return SHADE[kind]


def images(seed=418):
    """8 x 8, 1 x 1, 3 x 5, 1 x 1, 2 x 2, 2 x 2, 8 x 8, 3 x 5 (width x height): bytes and floats alternating"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (w, h) in enumerate(((8, 8), (1, 1), (3, 5), (1, 1), (2, 2), (2, 2), (8, 8), (3, 5))):
        out.append(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8) if k % 2 == 0 else rng.uniform(0, 1, size=(h, w, 4)).astype(F))
    return out


def texture_set(kind):
    """Seeded tangents for the first half of the shade data's triangles (every other one without: signs 0); bindings 0 both, 1
    albedo only, 2 normal only, 3 both with a negative scale, 4 neither."""
    if kind not in TEXTURES:
        shade = textured_shade(kind)
        rng = np.random.default_rng(4181 + len(kind))
        n_tan = shade.n_tris // 2
        t = rng.normal(size=(n_tan, 3, 3))
        t /= np.linalg.norm(t, axis=2)[:, :, None]
        sign = np.where(rng.random(n_tan) < 0.5, 1.0, -1.0)[:, None] * np.ones((1, 3))
        sign[::2] = 0
        tan = np.concatenate([t.reshape(n_tan, 9), sign], axis=1).astype(F)
        b = X.bindings([0, 7, None, 5, None], [3, None, 6, 2, None], [1.0, 2.0, 4.0, -0.5, 1.0])
        TEXTURES[kind] = X.TextureSet(images(), b, tan)
    return TEXTURES[kind]


def upload_shade(ctx, shade):
    ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)


def upload_textures(ctx, tex):
    ctx.upload_textures(tex.textures, tex.bindings, tex.tangents12)


def expected(rays, hits, shade, tex):
    rows, pairs, n = X.resolve_textured(rays["direction"], hits["normal"], hits["prim_id"] != -1, hits["prim_id"].view(np.uint32),
                                        hits["bary_u"], hits["bary_v"], shade, tex)
    out = hits.copy()
    out["normal"] = n
    return rows, pairs, out


class Out:
    """rows, pairs and records on the device with guard words behind each"""

    def __init__(self, dev, n, hit_bytes=32):
        self.dev, self.n, self.sizes = dev, n, (64, 8, hit_bytes)
        self.ptrs = [dev.put(np.full(n * size // 4 + GUARD, 0xA5A5A5A5, np.uint32)) for size in self.sizes]

    def check(self, want, hit_dtype=T.HIT32):
        rows, pairs, out = want
        got = [self.dev.get(p, self.n * size // 4 + GUARD, np.uint32) for p, size in zip(self.ptrs, self.sizes)]
        for g, size in zip(got, self.sizes):
            assert (g[self.n * size // 4:] == 0xA5A5A5A5).all()
        np.testing.assert_array_equal(got[0][:self.n * 16].reshape(-1, 16), words(rows).reshape(-1, 16))
        np.testing.assert_array_equal(got[1][:self.n * 2], words(pairs).reshape(-1))
        np.testing.assert_array_equal(got[2][:self.n * self.sizes[2] // 4], words(out).reshape(-1))

    def get(self):
        return [self.dev.get(p, self.n * size // 4, np.uint32) for p, size in zip(self.ptrs, self.sizes)]


def resolve_grid(run, flags=0):
    o = Out(run.dev, run.n)
    run.ctx.resolve_grid_surfaces(run.cam, run.w, run.h, run.d_hits, *o.ptrs, y0=run.y0, y1=run.y1, flags=flags)
    return o


def assert_cases_occur(hits, shade, tex):
    hit = hits["prim_id"] != -1
    prim = hits["prim_id"].view(np.uint32)
    in_range = hit & (prim < shade.n_tris)
    ids = np.where(in_range, prim % ID_PERIOD, NONE)
    tangent = in_range & (prim < tex.n_tangent_tris)
    signed = tangent & X.has_tangents(tex.tangents12[np.where(tangent, prim, 0)])
    assert (in_range & np.isin(ids, (0, 3)) & signed).any(), "both textures"
    assert (in_range & (ids == 1)).any(), "albedo only"
    assert (in_range & (ids == 2) & tangent & ~signed).any(), "normal only, tangents absent for the triangle"
    assert (in_range & (ids == 2) & signed).any(), "normal only"
    assert (in_range & (ids >= N_BINDINGS) & (ids < N_MATERIALS)).any(), "an id past n_bindings"
    assert (in_range & np.isin(ids, (0, 2, 3)) & ~tangent).any(), "a prim past n_tangent_tris"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_every_form_matches_the_restatement(built, kind, grid):
    """Grid form, array form, host-layout array form and in place: rows, d_bounce_surface and d_out_hits, byte for byte."""
    run = Run(kind, *grid)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade, tex = textured_shade(kind), texture_set(kind)
        assert_cases_occur(run.hits, shade, tex)
        upload_shade(ctx, shade)
        plain = resolve_grid(run).get()
        upload_textures(ctx, tex)
        want = expected(run.rays, run.hits, shade, tex)
        untextured = S.resolve(run.rays["direction"], run.hits["normal"], run.hits["prim_id"] != -1, run.hits["prim_id"].view(np.uint32),
                               run.hits["bary_u"], run.hits["bary_v"], shade)
        assert (words(want[0]["albedo"]) != words(untextured[0]["albedo"])).any(axis=1).sum() > n // 20
        assert (words(want[2]["normal"]) != words(untextured[2])).any(axis=1).sum() > n // 50
        np.testing.assert_array_equal(plain[0].reshape(-1, 16), words(untextured[0]).reshape(-1, 16))
        resolve_grid(run).check(want)
        # the array form on what mrt_cast read and wrote
        d_rays, d_h32 = dev.put(run.rays), dev.alloc(n * 32)
        ctx.cast(d_rays, d_h32, count=n, flags=DEV)
        same(dev.get(d_h32, n, T.HIT32), run.hits)
        o = Out(dev, n)
        ctx.resolve_surfaces(d_rays, d_h32, n, *o.ptrs)
        o.check(want)
        # the reference's host layout
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        rows44, pairs44, n44 = X.resolve_textured(hrays["direction"], h44["normal"], h44["prim_id"] != T.NO_HIT, h44["prim_id"], h44["u"], h44["v"], shade, tex)
        np.testing.assert_array_equal(words(rows44), words(want[0]))
        out44 = h44.copy()
        out44["normal"] = n44
        o = Out(dev, n, 44)
        ctx.resolve_surfaces(d_hr, d_h44, n, *o.ptrs, flags=capi.FLAG_HOST_LAYOUT)
        o.check((rows44, pairs44, out44), T.HOST_HIT44)
        # in place: d_out_hits may be d_hits itself
        ctx.resolve_surfaces(d_rays, d_h32, n, d_out_hits=d_h32)
        same(dev.get(d_h32, n, T.HIT32), want[2])
    finally:
        run.close()


def test_a_band_resolves_what_the_whole_frame_resolves(built):
    whole, band = Run("room", 128, 96), Run("room", 128, 96, 20, 70)
    try:
        rows = slice(20 * 128, 70 * 128)
        outs = []
        for run in (whole, band):
            upload_shade(run.ctx, textured_shade("room"))
            upload_textures(run.ctx, texture_set("room"))
            outs.append(resolve_grid(run).get())
        for a, b, size in zip(outs[0], outs[1], (16, 2, 8)):
            same(a.reshape(-1, size)[rows], b.reshape(-1, size))
    finally:
        whole.close()
        band.close()


@pytest.mark.parametrize("kind", ["soup", "room_tl"])
def test_no_binding_that_applies_equals_nothing_resident(built, kind):
    """A set whose every binding is MRT_NO_TEXTURE, a set without bindings, an empty set: the other kernel, the same bytes as the resolve
    with nothing resident; then the real set without UVs or ids resident: still the same bytes."""
    run = Run(kind, 100, 77)
    ctx = run.ctx
    try:
        shade, tex = textured_shade(kind), texture_set(kind)
        upload_shade(ctx, shade)
        plain = resolve_grid(run).get()
        none = X.bindings([None] * N_MATERIALS, [None] * N_MATERIALS, np.arange(N_MATERIALS))
        for t in (X.TextureSet(tex.textures, none, tex.tangents12), X.TextureSet(tex.textures, None, tex.tangents12), X.TextureSet()):
            upload_textures(ctx, t)
            for a, b in zip(resolve_grid(run).get(), plain):
                same(a, b)
        upload_textures(ctx, tex)
        assert any((a != b).any() for a, b in zip(resolve_grid(run).get(), plain))
        for absent in (S.ShadeData(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, None),
                       S.ShadeData(shade.n_tris, shade.materials, None, shade.normals9, shade.uvs6), None):
            if absent is None:
                ctx.clear_shade_data()
            else:
                upload_shade(ctx, absent)
            resolve_grid(run).check(expected(run.rays, run.hits, absent, tex))
            with_set = resolve_grid(run).get()
            ctx.clear_textures()
            for a, b in zip(with_set, resolve_grid(run).get()):
                same(a, b)
            upload_textures(ctx, tex)
    finally:
        run.close()


def test_a_uv_that_is_not_finite_samples_nothing(built):
    """Triangles with a NaN or an infinite vertex UV: their records get the unmultiplied albedo and the smooth normal."""
    run = Run("room", 100, 77)
    ctx = run.ctx
    try:
        shade, tex = textured_shade("room"), texture_set("room")
        uvs = shade.uvs6.copy()
        uvs[::3, 0, 0], uvs[1::3, 2, 1], uvs[4::9, 1, 0] = np.nan, np.inf, -np.inf
        bad = S.ShadeData(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, uvs)
        upload_shade(ctx, bad)
        plain = resolve_grid(run).get()
        upload_textures(ctx, tex)
        want = expected(run.rays, run.hits, bad, tex)
        k = ~np.isfinite(want[0]["uv"]).all(axis=1)
        assert k.sum() > run.n // 4 and (~k).sum() > run.n // 8
        o = resolve_grid(run)
        o.check(want)
        for a, b, size in zip(o.get(), plain, (16, 2, 8)):
            same(a.reshape(-1, size)[k], b.reshape(-1, size)[k])
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["soup", "room"])
def test_device_pointer_upload_resolves_identically(built, kind):
    """MRT_TEXTURES_ON_DEVICE: pixels and tangents copied device to device give the bytes of the host upload; with and without tangents."""
    run = Run(kind, 100, 77)
    ctx, dev = run.ctx, run.dev
    try:
        shade, tex = textured_shade(kind), texture_set(kind)
        upload_shade(ctx, shade)
        for tangents in (True, False):
            t = tex if tangents else X.TextureSet(tex.textures, tex.bindings, None)
            upload_textures(ctx, t)
            host = resolve_grid(run)
            host.check(expected(run.rays, run.hits, shade, t))
            ctx.clear_textures()
            on_dev = [(im.shape[1], im.shape[0], capi.TEXEL_RGBA8 if im.dtype == np.uint8 else capi.TEXEL_RGBA32F, dev.put(im)) for im in t.textures]
            ctx.upload_textures(on_dev, t.bindings, dev.put(t.tangents12) if tangents else None, t.n_tangent_tris, on_device=True)
            for a, b in zip(resolve_grid(run).get(), host.get()):
                same(a, b)
    finally:
        run.close()


def test_textures_survive_a_scene_upload_are_replaced_and_cleared(built):
    run = Run("room", 100, 77)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade, tex = textured_shade("room"), texture_set("room")
        upload_shade(ctx, shade)
        upload_textures(ctx, tex)
        want = expected(run.rays, run.hits, shade, tex)
        d_hits = dev.put(run.hits)                                            # the room's records, kept while the scene changes
        scene("soup").upload(ctx)
        scene("room").upload(ctx)
        ctx.refit_scene(capi.make_triangles(scene("room").verts, layers=scene("room").layers))
        o = Out(dev, n)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, d_hits, *o.ptrs)
        o.check(want)
        # replaced: other images (larger ones first: the pool grows), other bindings, fewer tangents
        other = X.TextureSet(images(7)[::-1] + [np.random.default_rng(3).uniform(0, 1, size=(16, 64, 4)).astype(F)],
                             X.bindings([8, None, 1, 2], [None, 4, 8, 0], [3.0, 1.0, 0.25, 1.0]), tex.tangents12[:tex.n_tangent_tris // 3])
        upload_textures(ctx, other)
        want2 = expected(run.rays, run.hits, shade, other)
        assert (words(want2[0]) != words(want[0])).any()
        o = Out(dev, n)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, d_hits, *o.ptrs)
        o.check(want2)
        upload_textures(ctx, tex)                                             # and back: a smaller pool in the larger buffer
        o = Out(dev, n)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, d_hits, *o.ptrs)
        o.check(want)
        ctx.clear_textures()
        o = Out(dev, n)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, d_hits, *o.ptrs)
        o.check(expected(run.rays, run.hits, shade, None))
        ctx.clear_textures()                                                  # nothing resident: still OK
        ctx.clear_shade_data()
        upload_textures(ctx, tex)                                             # a set without shade data: every hit as against nothing
        o = Out(dev, n)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, d_hits, *o.ptrs)
        o.check(expected(run.rays, run.hits, None, tex))
    finally:
        run.close()


COUNTS = {}


@pytest.mark.parametrize("count", [1, 255, 257, 2 ** 16 + 1])
def test_array_counts_and_guards(built, count):
    """The array form on the first `count` records of a 257 x 256 grid: one record, one short of a workgroup, one past it, one past
    2^16; the words behind every output keep their pattern and the inputs are read only."""
    run = Run("room", 257, 256)
    ctx, dev = run.ctx, run.dev
    try:
        shade, tex = textured_shade("room"), texture_set("room")
        upload_shade(ctx, shade)
        upload_textures(ctx, tex)
        d_rays = dev.put(run.rays)
        if "want" not in COUNTS:
            COUNTS["want"] = expected(run.rays[:2 ** 16 + 1], run.hits[:2 ** 16 + 1], shade, tex)
        o = Out(dev, count)
        ctx.resolve_surfaces(d_rays, run.d_hits, count, *o.ptrs)
        o.check(tuple(a[:count] for a in COUNTS["want"]))
        same(dev.get(run.d_hits, run.n, T.HIT32), run.hits)
        same(dev.get(d_rays, run.n, T.RAY32), run.rays)
    finally:
        run.close()


def test_async_then_synchronize(built):
    run = Run("soup", 100, 77)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade, tex = textured_shade("soup"), texture_set("soup")
        upload_shade(ctx, shade)
        upload_textures(ctx, tex)
        want = expected(run.rays, run.hits, shade, tex)
        d_rays = dev.put(run.rays)
        a = resolve_grid(run, flags=capi.FLAG_ASYNC)
        b = Out(dev, n)
        ctx.resolve_surfaces(d_rays, run.d_hits, n, *b.ptrs, flags=capi.FLAG_ASYNC)
        ctx.synchronize()
        a.check(want)
        b.check(want)
    finally:
        run.close()


def test_refusals_and_pending(built):
    """Every refusal of mrt_upload_textures, with and without a scene, with and without a set resident: MRT_ERR_INVALID and the resident
    set as it was; MRT_ERR_PENDING while a dispatch is pending."""
    L = capi.load()
    sc = scene("soup")
    w, h = 100, 77
    n = w * h
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        o, f, fov = sc.cam
        cam = capi.camera_look(o, f, w, h, fov)
        rays = po.grid_rays(o, f, w, h, fov)
        hits = sc.oracle(rays)
        d_hits = dev.put(hits)
        shade, tex = textured_shade("soup"), texture_set("soup")
        px = np.zeros((2, 2, 4), np.uint8)
        tan = np.zeros(12, F)
        size = C.sizeof(capi.TextureSet)

        def call(struct_size=size, flags=0, textures=((2, 2, 0, px.ctypes.data),), bindings=((0, NONE, 1.0),), n_textures=None, n_bindings=None,
                 n_tan=1, tangents=tan.ctypes.data, null_textures=False, null_bindings=False):
            t = (capi.Texture * max(len(textures), 1))(*[capi.Texture(tw, th, fmt, 0, p) for tw, th, fmt, p in textures])
            b = np.zeros(max(len(bindings), 1), T.MATERIAL_TEXTURES)
            for k, (a, nm, s) in enumerate(bindings):
                b[k] = (a, nm, s, 0)
            d = capi.TextureSet(struct_size, flags, len(textures) if n_textures is None else n_textures, len(bindings) if n_bindings is None else n_bindings,
                                n_tan, 0, None if null_textures else C.cast(t, C.c_void_p).value, None if null_bindings else b.ctypes.data, tangents)
            return L.mrt_upload_textures(ctx.h, C.byref(d))

        def bad_calls():
            assert L.mrt_upload_textures(ctx.h, None) == capi.ERR_INVALID
            for kw in (dict(struct_size=size + 8), dict(struct_size=0), dict(flags=2), dict(flags=1 << 31), dict(null_textures=True),
                       dict(null_bindings=True), dict(tangents=None), dict(textures=((0, 2, 0, px.ctypes.data),)),
                       dict(textures=((2, T.TEXTURE_MAX_DIM + 1, 0, px.ctypes.data),)), dict(textures=((2, 2, 2, px.ctypes.data),)),
                       dict(textures=((2, 2, 1, None),)), dict(bindings=((1, NONE, 1.0),)), dict(bindings=((NONE, 0xFFFFFFFE, 1.0),)),
                       dict(bindings=((0, 0, np.nan),)), dict(bindings=((0, 0, np.inf),)), dict(n_textures=0, null_textures=True),
                       dict(textures=((T.TEXTURE_MAX_DIM, T.TEXTURE_MAX_DIM, 1, px.ctypes.data),) * 16, bindings=())):
                assert call(**kw) == capi.ERR_INVALID, kw
                assert L.mrt_last_error(ctx.h) != b""

        def resolved():
            out = Out(dev, n)
            ctx.resolve_grid_surfaces(cam, w, h, d_hits, *out.ptrs)
            return out

        bad_calls()                                   # no scene, nothing resident
        resolved().check(expected(rays, hits, None, None))
        upload_shade(ctx, shade)
        upload_textures(ctx, tex)
        want = expected(rays, hits, shade, tex)
        bad_calls()                                   # a refused upload leaves the resident set as it was
        resolved().check(want)
        sc.upload(ctx)
        bad_calls()
        resolved().check(want)
        assert call(n_tan=0, tangents=None) == capi.MRT_OK          # a good one replaces it
        assert any((a != b).any() for a, b in zip(resolved().get(), [words(x).reshape(-1) for x in want]))
        upload_textures(ctx, tex)
        # a pending dispatch
        ctx.submit(rays)
        assert call() == capi.ERR_PENDING and L.mrt_clear_textures(ctx.h) == capi.ERR_PENDING
        ctx.collect()
        resolved().check(want)
        assert L.mrt_clear_textures(ctx.h) == capi.MRT_OK
    finally:
        dev.free()
        ctx.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_chain_into_lighting_and_the_path_step(built, kind):
    """Textured resolve, then mrt_light_grid_surfaces, then mrt_path_grid_step at bounce 0: lighting.py and path.py fed the textured rows
    and the perturbed normals."""
    run = Run(kind, 128, 96)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade, tex = textured_shade(kind), texture_set(kind)
        upload_shade(ctx, shade)
        upload_textures(ctx, tex)
        rows, pairs, shits = expected(run.rays, run.hits, shade, tex)
        o = resolve_grid(run)
        o.check((rows, pairs, shits))
        d_rows, _, d_shits = o.ptrs
        lights, env = light_list(kind), environment()
        d_mask, d_direct = dev.alloc(16 * n), dev.alloc(n * 16)
        ctx.cast_grid_shadows(run.cam, run.w, run.h, run.d_hits, capi.shadow_lights(lights), d_mask)
        mask = dev.get(d_mask, 16 * n, np.uint8)
        ctx.light_grid_surfaces(run.cam, run.w, run.h, run.d_hits, d_rows, lights, d_direct, d_mask, None)
        hit = run.hits["prim_id"] != -1
        direct = Lg.shade_linear(rows, hit, hit_point(run.rays, run.hits), run.rays["direction"], lights, mask.reshape(16, -1), None)[0]
        np.testing.assert_array_equal(words(dev.get(d_direct, n * 4, F).reshape(-1, 4)), words(direct))
        fresh = P.init_state(n)
        out = Outputs(dev, n, fresh)
        ctx.path_grid_step(run.cam, run.w, run.h, d_shits, d_rows, d_direct, out.d_state, env, out.d_select, FRAME, 0, 4, out.d_lobe, out.d_count)
        out.check(P.path_step(fresh, rows, hit, shits["normal"], run.rays["direction"], direct, env, np.arange(n, dtype=np.uint64), FRAME, 0, 4))
    finally:
        run.close()


def test_primary_grid_unaffected_by_textured_resolves(built):
    """A renderer's frames: the primary grid with and without texture uploads and textured resolves between frames -- the same kernel
    sequence, the same records."""
    sc = scene("room")
    w, h = 640, 480
    runs = []
    for resolving in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            upload_shade(ctx, textured_shade("room"))
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits, d_rows, d_pairs = dev.alloc(w * h * 32), dev.alloc(w * h * 64), dev.alloc(w * h * 8)
            for f in range(8):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, w * h, T.HIT32).view(np.uint32))
                if resolving:
                    if f % 3 == 0:
                        upload_textures(ctx, texture_set("room"))
                    ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows, d_pairs, flags=capi.FLAG_ASYNC if f & 1 else 0)
                    if f == 5:
                        ctx.synchronize()
                        ctx.clear_textures()
            runs.append((kernels, records))
        finally:
            dev.free()
            ctx.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)
