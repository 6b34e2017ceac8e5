"""mrt_cast_bounce / mrt_cast_grid_bounce: the path tracer's bounce (lobe choice, GGX half vector or cosine hemisphere) made in the
trace kernels from resident hit records, against the sampler restated in numpy float32 (messyerraytracer_amd/bounce.py; pinned to the
reference by test_bounce_cpu.py) and traced by the oracle -- rays, lobe bytes and records byte for byte.  A soup (back faces), flat
and two-level synth.room(); a per-record material pattern in which every lobe and the roughness clamp occur; grids on the plain lane
kernels (whole, ragged, a row band) and 2^16 records on the persistent ones; forced kernels; the diffuse lobe against
mrt_cast_hemisphere; constant materials; selection and query masks; a three-link chain; ASYNC; primary grids unaffected; errors."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import bounce as B
from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import hemisphere as H
from oracle import pyoracle as po
from test_hemisphere_gpu import DEV, PLACEHOLDER_HIT, Dev, Run, hit_point, same, scene, shadow_mask

pytestmark = pytest.mark.gpu

F = np.float32
FAR = F(1e30)
FRAME = 3
METALLIC, ROUGHNESS = np.array([0.0, 0.5, 1.0], F), np.array([0.02, 0.3, 1.0], F)   # 0.02: below the clamp


def surface(n):
    """{metallic, roughness} per record: metallic cycles fastest, all nine pairs occur"""
    i = np.arange(n)
    return np.stack([METALLIC[i % 3], ROUGHNESS[(i // 3) % 3]], axis=1).astype(F)


def expected(run, first_draw=0, frame=FRAME, surf=None, select=None, grid=True, t_max=FAR, metallic=0.0, roughness=0.5):
    """the restated rays, which entries have one and the lobe bytes.  grid: the pixel index is that of the whole grid; else the record's
    index (the array form).  surf None: the two constants."""
    pixel = np.arange(run.n, dtype=np.uint64) + (run.y0 * run.w if grid else 0)
    m, r = (metallic, roughness) if surf is None else (surf[:, 0], surf[:, 1])
    return B.bounce_rays(run.rays["direction"], hit_point(run.rays, run.hits), run.hits["normal"], run.hits["prim_id"] != -1, pixel,
                         frame, first_draw, t_max, m, r, select)


def specular_below_surface(run, surf, grid=True):
    """entries that are hits, drew the specular lobe and got no ray: at least one must occur"""
    pixel = np.arange(run.n, dtype=np.uint64) + (run.y0 * run.w if grid else 0)
    seed = H._u32(H._u32(pixel * np.uint64(1009)) + np.uint64((FRAME * 6529 + 7) & H.M32))
    m, ro = B.clamp_surface(surf[:, 0], surf[:, 1])
    spec = H.to_float(B.draw(seed, 0)) < B.spec_prob(m, ro)
    _, traced, _ = expected(run, surf=surf, grid=grid)
    return (run.hits["prim_id"] != -1) & spec & ~traced


def grid_cast(run, surf=None, first_draw=0, frame=FRAME, select=None, query_mask=0xFFFFFFFF, flags=0, t_max=FAR, metallic=0.0, roughness=0.5):
    """mrt_cast_grid_bounce: device pointers of the records, the rays and the lobe bytes"""
    dev = run.dev
    d_out, d_orays, d_lobe = dev.alloc(run.n * 32), dev.alloc(run.n * 32), dev.alloc(run.n)
    run.ctx.cast_grid_bounce(run.cam, run.w, run.h, run.d_hits, d_out, frame=frame, first_draw=first_draw, t_max=t_max, metallic=metallic,
                             roughness=roughness, d_select=None if select is None else dev.put(select.astype(np.uint8)),
                             d_surface=None if surf is None else dev.put(surf), d_out_lobe=d_lobe, d_out_rays=d_orays, y0=run.y0, y1=run.y1,
                             query_mask=query_mask, flags=flags)
    return d_out, d_orays, d_lobe


def check_all_entry_points(kind, w, h, y0=0, y1=None, kernel=capi.KERNEL_AUTO, variant=None):
    """The grid form and the array form in both layouts on one grid of one scene: rays, lobe bytes and records against the restated
    sampler traced by the oracle, byte for byte.  variant: a format with the source for the kernel every cast must report."""
    run = Run(kind, w, h, y0, y1, kernel)
    ctx, dev, n, sc = run.ctx, run.dev, run.n, run.sc
    surf = surface(n)

    def named(src):
        if variant:
            assert ctx.last_kernel_variant().startswith(variant % src), ctx.last_kernel_variant()

    try:
        for grid in (True, False):
            want_rays, traced, lobe = expected(run, surf=surf, grid=grid)
            hit = run.hits["prim_id"] != -1
            assert (lobe[hit] == B.LOBE_SPECULAR).mean() >= 0.05 and (lobe[hit] == B.LOBE_DIFFUSE).mean() >= 0.05
            assert specular_below_surface(run, surf, grid).any()
            assert (lobe != B.LOBE_NONE).tolist() == traced.tolist()
            want = sc.oracle(want_rays)
            assert (want["prim_id"][traced] != -1).any()
            same(want[~traced], np.repeat(PLACEHOLDER_HIT, (~traced).sum()))   # entries without a ray: the placeholder's record
            same(want_rays[~traced], np.repeat(H.PLACEHOLDER, (~traced).sum()))
            if kind == "soup":
                assert (~hit).any()
            if grid:
                d_out, d_orays, d_lobe = grid_cast(run, surf)
                named(12)
                same(dev.get(d_orays, n, T.RAY32), want_rays)
                np.testing.assert_array_equal(dev.get(d_lobe, n, np.uint8), lobe)
                same(dev.get(d_out, n, T.HIT32), want)
                continue
            # 32-byte records written by mrt_cast for the same rays
            d_rays, d_h32, d_surf = dev.put(run.rays), dev.alloc(n * 32), dev.put(surf)
            ctx.cast(d_rays, d_h32, count=n, flags=DEV)
            d_out2, d_orays2, d_lobe2 = dev.alloc(n * 32), dev.alloc(n * 32), dev.alloc(n)
            ctx.cast_bounce(d_rays, d_h32, n, d_out2, frame=FRAME, d_surface=d_surf, d_out_lobe=d_lobe2, d_out_rays=d_orays2)
            named(10)
            same(dev.get(d_orays2, n, T.RAY32), want_rays)
            np.testing.assert_array_equal(dev.get(d_lobe2, n, np.uint8), lobe)
            same(dev.get(d_out2, n, T.HIT32), want)
            # the reference's host layout: Ray / Intersection records in, Ray / Intersection out
            hrays = po.make_host_rays(run.rays)
            d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
            ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
            h44 = dev.get(d_h44, n, T.HOST_HIT44)
            rays44, _, lobe44 = B.bounce_rays(hrays["direction"], h44["position"], h44["normal"], h44["prim_id"] != T.NO_HIT, np.arange(n),
                                              FRAME, 0, FAR, surf[:, 0], surf[:, 1])
            same(rays44, want_rays)  # the record's position is o + d * t too
            d_out3, d_orays3, d_lobe3 = dev.alloc(n * 44), dev.alloc(n * 60), dev.alloc(n)
            ctx.cast_bounce(d_hr, d_h44, n, d_out3, frame=FRAME, d_surface=d_surf, d_out_lobe=d_lobe3, d_out_rays=d_orays3,
                            flags=capi.FLAG_HOST_LAYOUT)
            named(11)
            host_want_rays = po.make_host_rays(want_rays)
            same(dev.get(d_orays3, n, T.HOST_RAY60), host_want_rays)
            np.testing.assert_array_equal(dev.get(d_lobe3, n, np.uint8), lobe)
            same(dev.get(d_out3, n, T.HOST_HIT44), po.unpack_hits(want, host_want_rays))
    finally:
        run.close()


GRIDS = [(128, 96, 0, 96), (100, 77, 0, 77), (128, 96, 20, 70)]   # below 2^16 records
PLAIN = {"room": "trace_bounce_lane_kernel<%d>", "room_tl": "trace_bounce_two_level_kernel<%d>", "soup": "trace_bounce_lane_kernel<%d>",
         "affine_tl": "trace_bounce_two_level_kernel<%d>"}


@pytest.mark.parametrize("kind", ["soup", "room", "room_tl"])
@pytest.mark.parametrize("grid", GRIDS, ids=["128x96", "100x77", "band"])
def test_bounce_matches_the_oracle(built, kind, grid):
    check_all_entry_points(kind, *grid, variant=PLAIN[kind])


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_large_batch_runs_the_persistent_kernels(built, kind):
    """256 x 256 = 2^16 records: the persistent kernels (8-wide; two-level: 8-wide BLASes), every source."""
    check_all_entry_points(kind, 256, 256, variant="trace_bounce_persistent_kernel<%d, 8, " + ("true>" if kind == "room_tl" else "false>"))


@pytest.mark.parametrize("kind, kernel, variant", [
    ("room", capi.KERNEL_LANE, "trace_bounce_lane_kernel<%d>"),
    ("room", capi.KERNEL_LANE8_PERSISTENT, "trace_bounce_persistent_kernel<%d, 8, false>"),
    ("room", capi.KERNEL_LANE4_PERSISTENT, "trace_bounce_persistent_kernel<%d, 4, false>"),
    ("room", capi.KERNEL_LANE_PERSISTENT, "trace_bounce_persistent_kernel<%d, 2, false>"),
    ("room", capi.KERNEL_PACKET_ASM, "trace_bounce_persistent_kernel<%d, "),
    ("room_tl", capi.KERNEL_LANE, "trace_bounce_two_level_kernel<%d>"),
    ("room_tl", capi.KERNEL_PACKET_ASM, "trace_bounce_persistent_kernel<%d, 8, true>")],
    ids=["lane", "lane8p", "lane4p", "lane2p", "packet", "tl-lane", "tl-packet"])
def test_forced_kernels(built, kind, kernel, variant):
    """A forced kernel on 2^16 records; a forced packet kernel falls back to the policy's lane kernel.  (The two-level 2-wide
    persistent form is the policy's choice only for a scene without 8-wide meshes, which no upload path here produces: the policy
    driver pins that plan, the kernel shares its body with the forms run here.)"""
    check_all_entry_points(kind, 256, 256, kernel=kernel, variant=variant)


def test_a_row_band_draws_what_the_whole_frame_draws(built):
    """The seed uses the whole-grid pixel index; d_surface and d_out_lobe are indexed by the record within the band."""
    whole, band = Run("room", 128, 96), Run("room", 128, 96, 20, 70)
    try:
        rows = slice(20 * 128, 70 * 128)
        surf = surface(whole.n)
        outs = []
        for run, s in ((whole, surf), (band, surf[rows])):
            d_out, d_orays, d_lobe = grid_cast(run, s)
            outs.append((run.dev.get(d_out, run.n, T.HIT32), run.dev.get(d_orays, run.n, T.RAY32), run.dev.get(d_lobe, run.n, np.uint8)))
        for a, b in zip(outs[0], outs[1]):
            same(a[rows], b)
        assert len(set(outs[1][2].tolist())) == 3
    finally:
        whole.close()
        band.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
@pytest.mark.parametrize("first_draw", [0, 4])
def test_diffuse_entries_equal_the_hemisphere_cast(built, kind, first_draw):
    """Records and rays of diffuse-lobe entries are what mrt_cast_hemisphere(n_samples = 1, first_draw + 1) writes for them."""
    run = Run(kind, 128, 96)
    try:
        n, surf = run.n, surface(run.n)
        d_out, d_orays, d_lobe = grid_cast(run, surf, first_draw=first_draw)
        d_hout, d_hrays = run.dev.alloc(n * 32), run.dev.alloc(n * 32)
        run.ctx.cast_grid_hemisphere(run.cam, run.w, run.h, run.d_hits, d_hout, n_samples=1, frame=FRAME, first_draw=first_draw + 1,
                                     d_out_rays=d_hrays)
        diffuse = run.dev.get(d_lobe, n, np.uint8) == B.LOBE_DIFFUSE
        assert diffuse.mean() > 0.05
        same(run.dev.get(d_orays, n, T.RAY32)[diffuse], run.dev.get(d_hrays, n, T.RAY32)[diffuse])
        same(run.dev.get(d_out, n, T.HIT32)[diffuse], run.dev.get(d_hout, n, T.HIT32)[diffuse])
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_constant_material_equals_a_filled_surface_array(built, kind):
    run = Run(kind, 128, 96)
    try:
        n = run.n
        for metallic, roughness in ((0.0, 0.5), (1.0, 0.3), (0.5, 0.0), (1.0, 1.0)):
            filled = np.tile(np.array([metallic, roughness], F), (n, 1))
            a, b = grid_cast(run, None, metallic=metallic, roughness=roughness), grid_cast(run, filled, metallic=0.25, roughness=0.75)
            want_rays, traced, lobe = expected(run, metallic=metallic, roughness=roughness)
            assert traced.any()
            same(run.dev.get(a[1], n, T.RAY32), want_rays)
            np.testing.assert_array_equal(run.dev.get(a[2], n, np.uint8), lobe)
            for x, y, dt in zip(a, b, (T.HIT32, T.RAY32, np.uint8)):
                same(run.dev.get(x, n, dt), run.dev.get(y, n, dt))
    finally:
        run.close()


def test_nan_in_the_surface_array_takes_the_lower_bounds(built):
    run = Run("room", 64, 48)
    try:
        n = run.n
        surf = surface(n)
        surf[::2] = np.nan
        clamped = surf.copy()
        clamped[::2] = (0.0, 0.04)
        want_rays, traced, lobe = expected(run, surf=clamped)
        d_out, d_orays, d_lobe = grid_cast(run, surf)
        same(run.dev.get(d_orays, n, T.RAY32), want_rays)
        np.testing.assert_array_equal(run.dev.get(d_lobe, n, np.uint8), lobe)
        same(run.dev.get(d_out, n, T.HIT32), run.sc.oracle(want_rays))
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
@pytest.mark.parametrize("size", [(64, 48), (256, 256)], ids=["plain", "persistent"])
def test_selection_masks(built, kind, size):
    """A seeded random mask and an all-zero one: unselected records hold the placeholder's record and ray and the lobe byte 0."""
    run = Run(kind, *size)
    try:
        n, surf = run.n, surface(run.n)
        rng = np.random.default_rng(7)
        for sel in (rng.random(n) < 0.4, np.zeros(n, dtype=bool)):
            want_rays, traced, lobe = expected(run, surf=surf, select=sel)
            want = run.sc.oracle(want_rays)
            assert not traced[~sel].any() and (lobe[~sel] == B.LOBE_NONE).all()
            d_out, d_orays, d_lobe = grid_cast(run, surf, select=sel)
            same(run.dev.get(d_orays, n, T.RAY32), want_rays)
            np.testing.assert_array_equal(run.dev.get(d_lobe, n, np.uint8), lobe)
            same(run.dev.get(d_out, n, T.HIT32), want)
            same(want[~traced], np.repeat(PLACEHOLDER_HIT, (~traced).sum()))
        assert not traced.any()
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_query_mask_leaves_the_walls_out(built, kind):
    run = Run(kind, 128, 96)
    try:
        n, surf = run.n, surface(run.n)
        want_rays, traced, lobe = expected(run, surf=surf)
        want_all, want_obj = run.sc.oracle(want_rays), run.sc.oracle(want_rays, 1)
        assert (want_obj["prim_id"] != want_all["prim_id"]).any() and (want_obj["prim_id"] != -1).any()   # (walls: layer 2)
        d_out, d_orays, d_lobe = grid_cast(run, surf, query_mask=1)
        same(run.dev.get(d_out, n, T.HIT32), want_obj)
        same(run.dev.get(d_orays, n, T.RAY32), want_rays)   # (the mask filters what the ray may hit, not the ray)
        np.testing.assert_array_equal(run.dev.get(d_lobe, n, np.uint8), lobe)
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_three_link_chain(built, kind):
    """The reference's loop by queueing casts: bounce 0 (first_draw 0), shadows at the bounced points, bounce 1 (first_draw 3) from the
    first one's records and rays with the paths that ended switched off through d_select; each link held to the CPU."""
    run = Run(kind, 96, 72)
    ctx, dev, n, sc = run.ctx, run.dev, run.n, run.sc
    try:
        surf = surface(n)
        rays1, traced1, lobe1 = expected(run, surf=surf)
        hits1 = sc.oracle(rays1)
        d_out, d_orays, d_lobe = grid_cast(run, surf)
        same(dev.get(d_out, n, T.HIT32), hits1)
        lights = np.zeros(2, dtype=T.LIGHT)
        lights["cast_shadows"] = 1
        lights[0]["type"], lights[0]["position"] = T.LIGHT_POINT, (1.0, 4.5, 1.5)
        lights[1]["type"], lights[1]["direction"] = T.LIGHT_DIRECTIONAL, (0.3, 1.0, 0.2)
        want_mask = shadow_mask(sc, rays1, hits1, lights)
        assert want_mask.min() == 0 and want_mask.max() == 1
        d_mask = dev.alloc(2 * n)
        ctx.cast_shadows(d_orays, d_out, n, lights, d_mask)
        np.testing.assert_array_equal(dev.get(d_mask, 2 * n, np.uint8), want_mask)
        # the second bounce: record i keeps pixel i's stream (array form: the record's index), three draws on; a path without a first
        # bounce is switched off (its record is the placeholder's miss anyway), as one killed by roulette would be
        alive = lobe1 != B.LOBE_NONE
        surf2 = surface(n)[::-1].copy()
        rays2, traced2, lobe2 = B.bounce_rays(rays1["direction"], hit_point(rays1, hits1), hits1["normal"], hits1["prim_id"] != -1,
                                              np.arange(n), FRAME, 3, FAR, surf2[:, 0], surf2[:, 1], alive)
        hits2 = sc.oracle(rays2)
        assert traced2.any() and (hits2["prim_id"] != -1).any() and len(set(lobe2.tolist())) == 3
        d_out2, d_orays2, d_lobe2 = dev.alloc(n * 32), dev.alloc(n * 32), dev.alloc(n)
        ctx.cast_bounce(d_orays, d_out, n, d_out2, frame=FRAME, first_draw=3, d_select=d_lobe, d_surface=dev.put(surf2),
                        d_out_lobe=d_lobe2, d_out_rays=d_orays2)
        same(dev.get(d_orays2, n, T.RAY32), rays2)
        np.testing.assert_array_equal(dev.get(d_lobe2, n, np.uint8), lobe2)
        same(dev.get(d_out2, n, T.HIT32), hits2)
    finally:
        run.close()


def test_async_grid_then_async_bounce(built):
    run = Run("room", 160, 120)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        surf = surface(n)
        want_rays, _, lobe = expected(run, surf=surf)
        want = run.sc.oracle(want_rays)
        d_hits2, d_out, d_lobe, d_surf = dev.alloc(n * 32), dev.alloc(n * 32), dev.alloc(n), dev.put(surf)
        ctx.cast_grid(run.cam, run.w, run.h, hits=d_hits2, flags=capi.FLAG_HITS_ON_DEVICE | capi.FLAG_ASYNC)
        ctx.cast_grid_bounce(run.cam, run.w, run.h, d_hits2, d_out, frame=FRAME, d_surface=d_surf, d_out_lobe=d_lobe, flags=capi.FLAG_ASYNC)
        ctx.synchronize()
        same(dev.get(d_out, n, T.HIT32), want)
        np.testing.assert_array_equal(dev.get(d_lobe, n, np.uint8), lobe)
    finally:
        run.close()


def test_primary_grid_unaffected_by_bounce_casts(built):
    """A renderer's frames: the primary grid (scheduled from the second frame on: 2^17 rays and more) with and without bounce casts
    between frames -- the same kernel sequence (what the tuner and the tile schedules chose), the same records."""
    sc = scene("room")
    w, h = 640, 480
    runs = []
    for bounce in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits, d_out, d_rays = dev.alloc(w * h * 32), dev.alloc(w * h * 32), dev.alloc(w * h * 32)
            d_surf = dev.put(surface(w * h))
            for f in range(14):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, w * h, T.HIT32).view(np.uint32))
                if bounce:
                    ctx.cast_grid_bounce(cam, w, h, d_hits, d_out, frame=f, d_surface=d_surf, d_out_rays=d_rays)
                    if f & 1:
                        ctx.cast_bounce(d_rays, d_out, w * h, d_hits, frame=f, first_draw=3, d_surface=d_surf)
            runs.append((kernels, records))
        finally:
            dev.free()
            ctx.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)


def test_errors(built):
    L = capi.load()
    sc = scene("room")
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        w, h = 64, 48
        n = w * h
        cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
        d_rays, d_hits, d_out, d_orays = dev.alloc(n * 60), dev.alloc(n * 44), dev.alloc(n * 44), dev.alloc(n * 60)
        d_surf = dev.put(surface(n))
        R, Hp, O, OR = C.c_void_p(d_rays), C.c_void_p(d_hits), C.c_void_p(d_out), C.c_void_p(d_orays)
        pattern = np.full(n * 44, 7, np.uint8)
        ctx.h2d(d_out, pattern)

        def desc(t_max=10.0, metallic=0.5, roughness=0.5, surf=None):
            return capi.Bounce(0, 0, t_max, metallic, roughness, None, surf, None)

        def arr(rays=R, hits=Hp, count=n, d=None, out=O, orays=None, flags=0, no_desc=False):
            d = desc() if d is None else d
            return L.mrt_cast_bounce(ctx.h, rays, hits, count, None if no_desc else C.byref(d), out, orays, 0xFFFFFFFF, flags)

        def grid(hits=Hp, d=None, out=O, orays=None, flags=0, camera=cam, y0=0, y1=h, no_desc=False):
            d = desc() if d is None else d
            return L.mrt_cast_grid_bounce(ctx.h, C.byref(camera) if camera is not None else None, w, h, y0, y1, hits,
                                          None if no_desc else C.byref(d), out, orays, 0xFFFFFFFF, flags)

        bad_numbers = (float("nan"), float("inf"), -float("inf"), -0.01, 1.01)

        def bad_calls():
            common = [dict(hits=None), dict(out=None), dict(no_desc=True)]
            common += [dict(d=desc(t_max=t)) for t in (float("nan"), float("inf"), -float("inf"), 1e-4, 0.0, -1.0)]
            common += [dict(d=desc(metallic=x)) for x in bad_numbers] + [dict(d=desc(roughness=x)) for x in bad_numbers]
            for kw in common + [dict(rays=None)]:
                assert arr(**kw) == capi.ERR_INVALID, kw
            for kw in common + [dict(camera=None), dict(y0=10, y1=5), dict(y1=h + 1), dict(flags=capi.FLAG_HOST_LAYOUT)]:
                assert grid(**kw) == capi.ERR_INVALID, kw
            for f in (capi.FLAG_BOOL_OUT, capi.FLAG_TOKEN_OUT, capi.FLAG_COHERENT, capi.FLAG_FORCE_SORT, 1 << 20):
                assert arr(flags=f) == capi.ERR_INVALID and grid(flags=f) == capi.ERR_INVALID, f

        bad_calls()   # before a scene is uploaded: the arguments are checked first
        assert arr() == capi.ERR_NO_SCENE and grid() == capi.ERR_NO_SCENE and arr(count=0) == capi.ERR_NO_SCENE
        sc.upload(ctx)
        bad_calls()
        assert arr(count=0) == capi.MRT_OK  # nothing to do
        assert (dev.get(d_out, n * 44, np.uint8) == 7).all()  # no call so far wrote anything
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        assert grid() == capi.MRT_OK and grid(y0=10, y1=10) == capi.MRT_OK and grid(orays=OR) == capi.MRT_OK
        assert grid(d=desc(t_max=1.0001e-4, metallic=0.0, roughness=1.0)) == capi.MRT_OK
        # with a surface array the two constants are not read: any values pass
        assert grid(d=desc(metallic=float("nan"), roughness=7.0, surf=d_surf)) == capi.MRT_OK
        # pending work: a submitted dispatch must be collected first
        rays = po.grid_rays(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
        ctx.submit(rays)
        assert arr() == capi.ERR_PENDING and grid() == capi.ERR_PENDING
        ctx.collect()
        assert grid() == capi.MRT_OK
        d = desc()
        assert L.mrt_cast_bounce(None, R, Hp, n, C.byref(d), O, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
        assert L.mrt_cast_grid_bounce(None, C.byref(cam), w, h, 0, h, Hp, C.byref(d), O, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    finally:
        dev.free()
        ctx.close()
