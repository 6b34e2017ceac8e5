"""mrt_upload_shade_data / mrt_resolve_surfaces / mrt_resolve_grid_surfaces: hit records resolved to shading surfaces on the device
against the resident shade data, held to the numpy float32 restatement (messyerraytracer_amd/surface.py; pinned to the reference by
test_surface_cpu.py) byte for byte -- the 64-byte rows as uint32 words, the bounce pairs, the records with the shading normal.  A soup
(misses, back faces), flat and two-level synth.room(); seeded shade data in which the roughness clamp, an emitter, energy 0, material
ids out of range and prim ids out of range all occur among the hits of every grid; whole, ragged and band grids, 2^16 records; every
optional array absent in turn; device-array uploads; lifetime across scene uploads and a refit; the chains into mrt_cast_grid_bounce and
mrt_cast_grid_hemisphere; ASYNC; each output alone; errors; primary grids unaffected."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import hemisphere as H
from messyerraytracer_amd import surface as S
from oracle import pyoracle as po
from test_hemisphere_gpu import DEV, Dev, Run, hit_point, same, scene

pytestmark = pytest.mark.gpu

F = np.float32
FAR = F(1e30)
GRIDS = [(128, 96, 0, 96), (100, 77, 0, 77), (128, 96, 20, 70)]
GRID_IDS = ["128x96", "100x77", "band"]
KINDS = ["soup", "room", "room_tl"]
N_MATERIALS, ID_PERIOD, TRIS_LEFT_OUT = 7, 9, 7

SHADE = {}


def shade_data(kind):
    """Seeded shade data of a scene, made once: vertex normals = the face normal perturbed and renormalised per vertex; 7 materials
    (roughness below the clamp, an emitter, energy 0 with a colour); ids i % 9 (two of nine out of range); n_tris = the flat triangle
    count - 7 (the last prim ids out of range)."""
    if kind not in SHADE:
        v = np.ascontiguousarray(scene(kind).verts, dtype=np.float64).reshape(-1, 3, 3)
        n_flat = v.shape[0]
        rng = np.random.default_rng(4150 + len(kind))
        face = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        face /= np.maximum(np.linalg.norm(face, axis=1), 1e-30)[:, None]
        vn = face[:, None, :] + 0.35 * rng.normal(size=(n_flat, 3, 3))
        vn /= np.linalg.norm(vn, axis=2)[:, :, None]
        m = np.zeros(N_MATERIALS, T.MATERIAL)
        m["albedo"] = rng.uniform(0.05, 0.95, size=(N_MATERIALS, 3))
        m["metallic"] = [0.0, 0.5, 1.0, 0.25, 0.0, 1.0, 0.75]
        m["roughness"] = [0.02, 0.3, 1.0, 0.04, 0.0, 0.6, 0.039]        # 0.02, 0.0, 0.039: below the clamp
        m["specular"] = rng.uniform(0.0, 1.0, size=N_MATERIALS)
        m["emission"] = rng.uniform(0.0, 2.0, size=(N_MATERIALS, 3))
        m["emission_energy"] = [0.0, 3.5, 0.0, 0.0, 12.0, -1.0, 0.0]    # 1, 4: emitters; the rest: energy 0 (or below) with a colour
        m["flags"] = np.arange(N_MATERIALS) % 4
        n = n_flat - TRIS_LEFT_OUT
        SHADE[kind] = S.ShadeData(n, m, (np.arange(n) % ID_PERIOD).astype(np.uint32), vn[:n].astype(F), rng.uniform(-1, 2, size=(n, 3, 2)).astype(F))
    return SHADE[kind]


def without(shade, *absent):
    """the same shade data with some arrays absent: 'ids', 'normals', 'uvs', 'materials'"""
    return S.ShadeData(shade.n_tris, None if "materials" in absent else shade.materials, None if "ids" in absent else shade.material_ids,
                       None if "normals" in absent else shade.normals9, None if "uvs" in absent else shade.uvs6)


def upload(ctx, shade):
    ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)


def expected(rays, hits, shade):
    """rows, bounce pairs and the records with the shading normal, from mrt_ray32 rays and mrt_hit32 records"""
    rows, pairs, n = S.resolve(rays["direction"], hits["normal"], hits["prim_id"] != -1, hits["prim_id"].view(np.uint32),
                               hits["bary_u"], hits["bary_v"], shade)
    out = hits.copy()
    out["normal"] = n
    return rows, pairs, out


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(dev, n, d_rows, d_pairs, d_out, want, hit_dtype=T.HIT32):
    rows, pairs, out = want
    np.testing.assert_array_equal(words(dev.get(d_rows, n, T.SURFACE64)), words(rows))
    same(dev.get(d_pairs, n * 2, F), pairs.reshape(-1))
    same(dev.get(d_out, n, hit_dtype), out)


def resolve_grid(run, flags=0):
    d_rows, d_pairs, d_out = run.dev.alloc(run.n * 64), run.dev.alloc(run.n * 8), run.dev.alloc(run.n * 32)
    run.ctx.resolve_grid_surfaces(run.cam, run.w, run.h, run.d_hits, d_rows, d_pairs, d_out, y0=run.y0, y1=run.y1, flags=flags)
    return d_rows, d_pairs, d_out


def assert_cases_occur(kind, hits, shade):
    hit = hits["prim_id"] != -1
    prim = hits["prim_id"].view(np.uint32)
    in_range = hit & (prim < shade.n_tris)
    ids = np.where(in_range, prim % ID_PERIOD, 0)
    mat = in_range & (ids < N_MATERIALS)
    m = shade.materials[np.where(mat, ids, 0)]
    assert (mat & (m["roughness"] < F(0.04))).any(), "roughness below the clamp"
    assert (mat & (m["emission_energy"] > 0)).any(), "an emitter"
    assert (mat & (m["emission_energy"] == 0) & (m["emission"] != 0).any(axis=1)).any(), "energy 0 with a colour"
    assert (in_range & (ids >= N_MATERIALS)).any(), "a material id out of range"
    assert (hit & ~in_range).any(), "a prim id out of range"
    if kind == "soup":
        assert (~hit).any(), "misses"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_every_form_matches_the_restatement(built, kind, grid):
    """1. Grid form, array form and host-layout array form: rows, d_bounce_surface and d_out_hits, byte for byte."""
    run = Run(kind, *grid)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade = shade_data(kind)
        assert_cases_occur(kind, run.hits, shade)
        upload(ctx, shade)
        want = expected(run.rays, run.hits, shade)
        assert (words(want[2]["normal"]) != words(run.hits["normal"])).any()
        check(dev, n, *resolve_grid(run), want)
        # the array form on what mrt_cast read and wrote
        d_rays, d_h32 = dev.put(run.rays), dev.alloc(n * 32)
        ctx.cast(d_rays, d_h32, count=n, flags=DEV)
        same(dev.get(d_h32, n, T.HIT32), run.hits)
        d_rows, d_pairs, d_out = dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 32)
        ctx.resolve_surfaces(d_rays, d_h32, n, d_rows, d_pairs, d_out)
        check(dev, n, d_rows, d_pairs, d_out, want)
        # the reference's host layout
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        rows44, pairs44, n44 = S.resolve(hrays["direction"], h44["normal"], h44["prim_id"] != T.NO_HIT, h44["prim_id"], h44["u"], h44["v"], shade)
        np.testing.assert_array_equal(words(rows44), words(want[0]))
        out44 = h44.copy()
        out44["normal"] = n44
        d_rows3, d_pairs3, d_out3 = dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 44)
        ctx.resolve_surfaces(d_hr, d_h44, n, d_rows3, d_pairs3, d_out3, flags=capi.FLAG_HOST_LAYOUT)
        check(dev, n, d_rows3, d_pairs3, d_out3, (rows44, pairs44, out44), T.HOST_HIT44)
        # in place: d_out_hits may be d_hits itself
        ctx.resolve_surfaces(d_rays, d_h32, n, d_out_hits=d_h32)
        same(dev.get(d_h32, n, T.HIT32), want[2])
    finally:
        run.close()


def test_a_band_resolves_what_the_whole_frame_resolves(built):
    whole, band = Run("room", 128, 96), Run("room", 128, 96, 20, 70)
    try:
        shade = shade_data("room")
        rows = slice(20 * 128, 70 * 128)
        outs = []
        for run in (whole, band):
            upload(run.ctx, shade)
            d_rows, d_pairs, d_out = resolve_grid(run)
            outs.append((run.dev.get(d_rows, run.n, T.SURFACE64), run.dev.get(d_pairs, run.n * 2, F).reshape(-1, 2), run.dev.get(d_out, run.n, T.HIT32)))
        for a, b in zip(outs[0], outs[1]):
            same(a[rows], b)
    finally:
        whole.close()
        band.close()


@pytest.mark.parametrize("kind", ["soup", "room_tl"])
def test_absent_arrays_no_shade_data_and_clear(built, kind):
    """2. Each optional array absent in turn, several at once, then no shade data at all; mrt_clear_shade_data gives the same."""
    run = Run(kind, 100, 77)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        full = shade_data(kind)
        nothing = expected(run.rays, run.hits, None)
        same(nothing[2], run.hits)                                            # the face normal: the records as they were
        assert (nothing[0]["material"] == T.DEFAULT_MATERIAL).all()
        check(dev, n, *resolve_grid(run), nothing)                            # nothing resident yet
        for absent in (("ids",), ("normals",), ("uvs",), ("materials",), ("ids", "uvs"), ("normals", "uvs"), ("ids", "normals", "uvs")):
            shade = without(full, *absent)
            upload(ctx, shade)
            want = expected(run.rays, run.hits, shade)
            if "normals" in absent:
                same(want[2], run.hits)
            if "uvs" in absent:
                assert (want[0]["uv"] == 0).all()
            if "ids" in absent or "materials" in absent:
                assert (want[0]["material"] == T.DEFAULT_MATERIAL).all()
            check(dev, n, *resolve_grid(run), want)
        upload(ctx, S.ShadeData(0, full.materials))                           # n_tris 0: every prim id out of range
        check(dev, n, *resolve_grid(run), nothing)
        upload(ctx, full)
        check(dev, n, *resolve_grid(run), expected(run.rays, run.hits, full))
        ctx.clear_shade_data()
        check(dev, n, *resolve_grid(run), nothing)
        ctx.clear_shade_data()                                                # nothing resident: still OK
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["soup", "room"])
def test_device_array_upload_resolves_identically(built, kind):
    """3. MRT_SHADE_ARRAYS_ON_DEVICE: the rows packed by the kernel are the rows packed on the host."""
    run = Run(kind, 100, 77)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        full = shade_data(kind)
        for absent in ((), ("normals",), ("ids", "uvs")):
            shade = without(full, *absent)
            d = [None if a is None else dev.put(a) for a in (shade.material_ids, shade.normals9, shade.uvs6)]
            ctx.upload_shade_data(shade.n_tris, shade.materials, d[0], d[1], d[2], on_device=True)
            check(dev, n, *resolve_grid(run), expected(run.rays, run.hits, shade))
    finally:
        run.close()


def test_shade_data_survives_scene_uploads_and_a_refit(built):
    """4. The shade data is the context's: another scene's upload and a refit leave it; a second upload replaces it."""
    run = Run("room", 100, 77)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade = shade_data("room")
        upload(ctx, shade)
        want = expected(run.rays, run.hits, shade)
        d_hits = dev.put(run.hits)                                            # the room's records, kept while the scene changes
        scene("soup").upload(ctx)
        scene("room").upload(ctx)
        tris = capi.make_triangles(scene("room").verts, layers=scene("room").layers)
        ctx.refit_scene(tris)
        d_rows, d_pairs, d_out = dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 32)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, d_hits, d_rows, d_pairs, d_out)
        check(dev, n, d_rows, d_pairs, d_out, want)
        other = without(shade, "normals")
        other.materials = shade.materials[::-1].copy()
        upload(ctx, other)
        want2 = expected(run.rays, run.hits, other)
        assert (words(want2[0]) != words(want[0])).any()
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, d_hits, d_rows, d_pairs, d_out)
        check(dev, n, d_rows, d_pairs, d_out, want2)
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_bounce_cast_takes_the_kernels_pairs(built, kind):
    """5a. mrt_cast_grid_bounce with the kernel's d_bounce_surface equals the same cast with the host-computed array: rays, lobe
    bytes, records."""
    run = Run(kind, 128, 96)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade = shade_data(kind)
        upload(ctx, shade)
        _, pairs, _ = expected(run.rays, run.hits, shade)
        d_pairs = dev.alloc(n * 8)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, run.d_hits, d_bounce_surface=d_pairs)
        got = []
        for d_surface in (d_pairs, dev.put(pairs)):
            d_out, d_orays, d_lobe = dev.alloc(n * 32), dev.alloc(n * 32), dev.alloc(n)
            ctx.cast_grid_bounce(run.cam, run.w, run.h, run.d_hits, d_out, frame=3, t_max=FAR, d_surface=d_surface, d_out_lobe=d_lobe, d_out_rays=d_orays)
            got.append((dev.get(d_orays, n, T.RAY32), dev.get(d_lobe, n, np.uint8), dev.get(d_out, n, T.HIT32)))
        for a, b in zip(*got):
            same(a, b)
        assert len(set(got[0][1].tolist())) == 3
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_hemisphere_cast_takes_the_shading_normals(built, kind):
    """5b. mrt_cast_grid_hemisphere (nearest, 1 sample) fed d_out_hits equals hemisphere.py run on the smooth normals, traced by the oracle."""
    run = Run(kind, 128, 96)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade = shade_data(kind)
        upload(ctx, shade)
        _, _, out = expected(run.rays, run.hits, shade)
        d_smooth = dev.alloc(n * 32)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, run.d_hits, d_out_hits=d_smooth)
        d_out, d_orays = dev.alloc(n * 32), dev.alloc(n * 32)
        ctx.cast_grid_hemisphere(run.cam, run.w, run.h, d_smooth, d_out, n_samples=1, frame=3, first_draw=1, t_max=FAR, d_out_rays=d_orays)
        want_rays, traced, _ = H.hemisphere_rays(run.rays["direction"], hit_point(run.rays, run.hits), out["normal"], out["prim_id"] != -1,
                                                 np.arange(n, dtype=np.uint64), 1, 3, 1, FAR)
        flat_rays, _, _ = H.hemisphere_rays(run.rays["direction"], hit_point(run.rays, run.hits), run.hits["normal"], out["prim_id"] != -1,
                                            np.arange(n, dtype=np.uint64), 1, 3, 1, FAR)
        assert traced.any() and (words(want_rays) != words(flat_rays)).any()
        same(dev.get(d_orays, n, T.RAY32), want_rays)
        same(dev.get(d_out, n, T.HIT32), run.sc.oracle(want_rays))
    finally:
        run.close()


def test_async_then_synchronize(built):
    """6. MRT_FLAG_ASYNC followed by mrt_synchronize gives the same bytes, both forms."""
    run = Run("soup", 100, 77)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade = shade_data("soup")
        upload(ctx, shade)
        want = expected(run.rays, run.hits, shade)
        d_rays = dev.put(run.rays)
        a = resolve_grid(run, flags=capi.FLAG_ASYNC)
        b = dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 32)
        ctx.resolve_surfaces(d_rays, run.d_hits, n, *b, flags=capi.FLAG_ASYNC)
        ctx.synchronize()
        check(dev, n, *a, want)
        check(dev, n, *b, want)
    finally:
        run.close()


def test_outputs_alone_count_zero_and_errors(built):
    """7, 8 and the checks: each output pointer alone; all-null outputs, null pointers, unknown flags and bad grids are invalid, with
    and without a scene, before anything is written; count == 0 is OK and writes nothing; no scene is required."""
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
        d_rays, d_hits = dev.put(rays), dev.put(hits)
        pattern = np.full(n * 64, 7, np.uint8)
        d_a, d_b, d_c = dev.put(pattern), dev.put(pattern[:n * 8]), dev.put(pattern[:n * 32])
        R, Hp = C.c_void_p(d_rays), C.c_void_p(d_hits)
        all_out = capi.surface_out(d_a, d_b, d_c)

        def arr(rays=R, hits=Hp, count=n, out=all_out, flags=0):
            return L.mrt_resolve_surfaces(ctx.h, rays, hits, count, None if out is None else C.byref(out), flags)

        def grid(hits=Hp, out=all_out, flags=0, camera=cam, y0=0, y1=h):
            return L.mrt_resolve_grid_surfaces(ctx.h, None if camera is None else C.byref(camera), w, h, y0, y1, hits,
                                               None if out is None else C.byref(out), flags)

        def untouched():
            return (dev.get(d_a, n * 64, np.uint8) == 7).all() and (dev.get(d_b, n * 8, np.uint8) == 7).all() and (dev.get(d_c, n * 32, np.uint8) == 7).all()

        def bad_calls():
            common = [dict(hits=None), dict(out=None), dict(out=capi.surface_out())]
            for kw in common + [dict(rays=None)]:
                assert arr(**kw) == capi.ERR_INVALID, kw
            for kw in common + [dict(camera=None), dict(y0=10, y1=5), dict(y1=h + 1), dict(flags=capi.FLAG_HOST_LAYOUT)]:
                assert grid(**kw) == capi.ERR_INVALID, kw
            for fl in (capi.FLAG_BOOL_OUT, capi.FLAG_TOKEN_OUT, capi.FLAG_COHERENT, capi.FLAG_FORCE_SORT, capi.FLAG_RAYS_ON_DEVICE, 1 << 20):
                assert arr(flags=fl) == capi.ERR_INVALID and grid(flags=fl) == capi.ERR_INVALID, fl
            bad = capi.ShadeData(C.sizeof(capi.ShadeData), 1, 1, 0, None, None, None, None)          # n_materials > 0, null materials
            assert L.mrt_upload_shade_data(ctx.h, C.byref(bad)) == capi.ERR_INVALID
            assert L.mrt_upload_shade_data(ctx.h, None) == capi.ERR_INVALID
            m = np.zeros(1, T.MATERIAL)
            m["roughness"] = np.nan
            for d in (capi.ShadeData(C.sizeof(capi.ShadeData) + 8, 0, 0, 0, None, None, None, None),
                      capi.ShadeData(C.sizeof(capi.ShadeData), 0, 0, 2, None, None, None, None),
                      capi.ShadeData(C.sizeof(capi.ShadeData), 0, 1, 0, m.ctypes.data, None, None, None)):
                assert L.mrt_upload_shade_data(ctx.h, C.byref(d)) == capi.ERR_INVALID

        bad_calls()                                   # no scene, no shade data
        assert arr(count=0) == capi.MRT_OK and grid(y0=10, y1=10) == capi.MRT_OK
        assert untouched()
        # no scene is required: the defaults against nothing resident
        nothing = expected(rays, hits, None)
        assert grid() == capi.MRT_OK
        check(dev, n, d_a, d_b, d_c, nothing)
        shade = shade_data("soup")
        upload(ctx, shade)
        bad_calls()                                   # a refused upload leaves the resident data as it was
        want = expected(rays, hits, shade)
        assert arr() == capi.MRT_OK
        check(dev, n, d_a, d_b, d_c, want)
        sc.upload(ctx)
        bad_calls()
        # each output alone: the other two buffers keep their pattern
        for k, (nbytes, dtype, ref) in enumerate(((64, T.SURFACE64, want[0]), (8, np.dtype((F, 2)), want[1]), (32, T.HIT32, want[2]))):
            for p, size in ((d_a, 64), (d_b, 8), (d_c, 32)):
                ctx.h2d(p, pattern[:n * size])
            ptrs = [None, None, None]
            ptrs[k] = (d_a, d_b, d_c)[k]
            for call in (lambda: arr(out=capi.surface_out(*ptrs)), lambda: grid(out=capi.surface_out(*ptrs))):
                assert call() == capi.MRT_OK
                np.testing.assert_array_equal(words(dev.get(ptrs[k], n, dtype)), words(ref))
                for j, (p, size) in enumerate(((d_a, 64), (d_b, 8), (d_c, 32))):
                    if j != k:
                        assert (dev.get(p, n * size, np.uint8) == 7).all()
        # a pending dispatch
        ctx.submit(rays)
        good = capi.ShadeData(C.sizeof(capi.ShadeData), 0, 0, 0, None, None, None, None)
        assert arr() == capi.ERR_PENDING and grid() == capi.ERR_PENDING
        assert L.mrt_upload_shade_data(ctx.h, C.byref(good)) == capi.ERR_PENDING and L.mrt_clear_shade_data(ctx.h) == capi.ERR_PENDING
        ctx.collect()
        assert arr() == capi.MRT_OK
        check(dev, n, d_a, d_b, d_c, want)
    finally:
        dev.free()
        ctx.close()


def test_primary_grid_unaffected_by_resolves(built):
    """9. A renderer's frames: the primary grid with and without resolves between frames -- the same kernel sequence, the same records."""
    sc = scene("room")
    w, h = 640, 480
    runs = []
    for resolving in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            upload(ctx, shade_data("room"))
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits, d_rows, d_pairs = dev.alloc(w * h * 32), dev.alloc(w * h * 64), dev.alloc(w * h * 8)
            for f in range(8):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, w * h, T.HIT32).view(np.uint32))
                if resolving:
                    ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows, d_pairs, flags=capi.FLAG_ASYNC if f & 1 else 0)
            runs.append((kernels, records))
        finally:
            dev.free()
            ctx.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("kind", ["soup", "room_tl"])
def test_two_to_the_sixteen_records(built, kind):
    """10. 256 x 256 = 2^16 records."""
    run = Run(kind, 256, 256)
    try:
        shade = shade_data(kind)
        assert_cases_occur(kind, run.hits, shade)
        upload(run.ctx, shade)
        check(run.dev, run.n, *resolve_grid(run), expected(run.rays, run.hits, shade))
    finally:
        run.close()
