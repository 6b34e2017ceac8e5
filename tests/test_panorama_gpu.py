"""mrt_upload_panorama / mrt_clear_panorama and what the lighting calls and the path steps compute while a panorama is resident, held to
the numpy restatements (messyerraytracer_amd/panorama.py, lighting.py, path.py; pinned to the reference by test_panorama_cpu.py) as
uint32 words, byte for byte.  The scenes, grids, shade data, lights and environment of test_surface_gpu.py / test_lighting_gpu.py / the
chain of test_path_gpu.py; the images of panorama_cases.py.  Lighting: grid, array and host-layout forms on images of 1x1, 3x2, 64x32
and 257x129, 0 / 1 / 16 lights, with and without the mask; 1, 255, 257 and 2^16 + 1 records with guards; a band; ASYNC; hand-placed
rays and normals at the seam, the poles and texel edges; NaN directions; env == NULL, clear, replace, ON_DEVICE.  Path: bounce 0 and 1
in both forms, a two-bounce frame.  Refusals; the primary cast undisturbed."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import panorama as Pn
from messyerraytracer_amd import path as P
from oracle import pyoracle as po
from test_hemisphere_gpu import DEV, Dev, same, scene
from test_lighting_gpu import Lit, check, environment, light_list
from test_path_gpu import FRAME, Chain, Outputs, mixed_state
from test_panorama_cpu import fixture
from test_surface_gpu import shade_data, upload, words

pytestmark = pytest.mark.gpu

F = np.float32
FAR = F(1e30)
ENERGY = 1.75
IMAGE_NAMES = ["1x1", "3x2", "64x32", "257x129"]


def image(name):
    return fixture()["images"][name]


def want_lit(lit, pano, n_lights=16, mask=True, env=True):
    m = lit.mask.reshape(16, -1)[:n_lights] if mask else None
    return Lg.shade_linear(lit.rows, lit.hit, lit.p, lit.run.rays["direction"], lit.lights[:n_lights], m, lit.env if env else None,
                           panorama=pano)[0]


def assert_misses_hits_and_both_hemispheres(lit):
    ny = lit.rows["normal"][lit.hit, 1]
    assert lit.hit.any() and (~lit.hit).any() and (ny > 0.1).any() and (ny < -0.1).any()


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_lighting_forms_on_every_image(built, name):
    """Grid, array and host-layout forms with the panorama resident; the grid form with 0, 1 and 16 lights, with and without the mask;
    without an environment the panorama is not read."""
    lit = Lit("soup", 100, 77)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        assert_misses_hits_and_both_hemispheres(lit)
        pano = (image(name), ENERGY)
        ctx.upload_panorama(*pano)
        want = want_lit(lit, pano)
        assert np.isfinite(want).all() and (want[~lit.hit, :3] > 0).all() and (want[~lit.hit, 3] == 0).all() and (want[lit.hit, 3] == 1).all()
        assert (words(want) != words(lit.want())).any()                            # not the gradient's frame
        d_rgba = dev.alloc(n * 16)
        lit.grid(d_rgba)
        check(dev, d_rgba, want)
        for kw in (dict(mask=False), dict(n_lights=0), dict(n_lights=0, mask=False), dict(n_lights=1), dict(n_lights=1, mask=False)):
            lit.grid(d_rgba, **kw)
            check(dev, d_rgba, want_lit(lit, pano, **kw))
        for kw in (dict(env=False), dict(env=False, mask=False, n_lights=1)):
            lit.grid(d_rgba, **kw)
            check(dev, d_rgba, lit.want(**kw))                                      # env == NULL: today's output
        d_rays, d_out = dev.put(run.rays), dev.alloc(n * 16)
        ctx.light_surfaces(d_rays, run.d_hits, lit.d_rows, n, lit.lights, d_out, lit.d_mask, lit.env)
        check(dev, d_out, want)
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        d_rows44, d_mask44, d_out44 = dev.alloc(n * 64), dev.alloc(16 * n), dev.alloc(n * 16)
        ctx.resolve_surfaces(d_hr, d_h44, n, d_rows44, flags=capi.FLAG_HOST_LAYOUT)
        ctx.cast_shadows(d_hr, d_h44, n, capi.shadow_lights(lit.lights), d_mask44, flags=capi.FLAG_HOST_LAYOUT)
        rows44, mask44 = dev.get(d_rows44, n, T.SURFACE64), dev.get(d_mask44, 16 * n, np.uint8)
        want44 = Lg.shade_linear(rows44, h44["prim_id"] != T.NO_HIT, h44["position"], hrays["direction"], lit.lights, mask44.reshape(16, -1),
                                 lit.env, panorama=pano)[0]
        ctx.light_surfaces(d_hr, d_h44, d_rows44, n, lit.lights, d_out44, d_mask44, lit.env, flags=capi.FLAG_HOST_LAYOUT)
        check(dev, d_out44, want44)
    finally:
        lit.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_lighting_on_the_rooms(built, kind):
    lit = Lit(kind, 128, 96, 20, 70)
    try:
        pano = (image("64x32"), ENERGY)
        lit.run.ctx.upload_panorama(*pano)
        d = lit.run.dev.alloc(lit.run.n * 16)
        lit.grid(d)
        check(lit.run.dev, d, want_lit(lit, pano))
    finally:
        lit.close()


@pytest.mark.parametrize("count", [1, 255, 257, 2 ** 16 + 1])
def test_array_counts_and_guards(built, count):
    lit = Lit("soup", 257, 256)
    run = lit.run
    ctx, dev = run.ctx, run.dev
    try:
        pano = (image("257x129"), ENERGY)
        ctx.upload_panorama(*pano)
        d_rays = dev.put(run.rays)
        d_mask = dev.alloc(16 * count)
        ctx.cast_shadows(d_rays, run.d_hits, count, capi.shadow_lights(lit.lights), d_mask)
        mask = dev.get(d_mask, 16 * count, np.uint8).reshape(16, count)
        want = Lg.shade_linear(lit.rows[:count], lit.hit[:count], lit.p[:count], run.rays["direction"][:count], lit.lights, mask, lit.env,
                               panorama=pano)[0]
        guard = np.full((count + 64) * 4, -7.5, F)
        d_before, d_out, d_after = dev.put(guard[:256]), dev.put(guard), dev.put(guard[:256])
        bufs = ((lit.d_rows, run.n * 64), (run.d_hits, run.n * 32), (d_rays, run.n * 32), (d_mask, 16 * count))
        before = [dev.get(p, k, np.uint8) for p, k in bufs]
        ctx.light_surfaces(d_rays, run.d_hits, lit.d_rows, count, lit.lights, d_out, d_mask, lit.env)
        got = dev.get(d_out, (count + 64) * 4, F)
        np.testing.assert_array_equal(words(got[:count * 4].reshape(-1, 4)), words(want))
        assert (got[count * 4:] == F(-7.5)).all() and (dev.get(d_before, 256, F) == F(-7.5)).all() and (dev.get(d_after, 256, F) == F(-7.5)).all()
        for a, (p, k) in zip(before, bufs):
            np.testing.assert_array_equal(a, dev.get(p, k, np.uint8))               # the inputs are read only
    finally:
        lit.close()


def test_a_band_lights_what_the_whole_frame_lights_and_async(built):
    whole, band = Lit("soup", 128, 96), Lit("soup", 128, 96, 20, 70)
    try:
        pano = (image("64x32"), ENERGY)
        outs = []
        for lit in (whole, band):
            lit.run.ctx.upload_panorama(*pano)
            d = lit.run.dev.alloc(lit.run.n * 16)
            lit.grid(d, flags=capi.FLAG_ASYNC)
            lit.run.ctx.synchronize()
            outs.append(lit.run.dev.get(d, lit.run.n * 4, F).reshape(-1, 4))
        same(outs[0][20 * 128:70 * 128], outs[1])
        np.testing.assert_array_equal(words(outs[0]), words(want_lit(whole, pano)))
        assert_misses_hits_and_both_hemispheres(band)
        # ... the array form queued behind it
        run = whole.run
        d_rays, b = run.dev.put(run.rays), run.dev.alloc(run.n * 16)
        run.ctx.light_surfaces(d_rays, run.d_hits, whole.d_rows, run.n, whole.lights, b, whole.d_mask, whole.env, flags=capi.FLAG_ASYNC)
        run.ctx.synchronize()
        check(run.dev, b, want_lit(whole, pano))
    finally:
        whole.close()
        band.close()


def placed_records():
    """Array-form records placed by hand, no scene: the fixture's pole, seam, texel-edge and outside directions once as the rays of
    misses and once as the row normals of hits, with a few non-finite ones between them."""
    g = fixture()
    gr = g["groups"]
    d = np.concatenate([g["directions"][slice(*gr[k])] for k in ("poles", "seam", "edges", "outside")] + [g["directions"][:255]])
    d = d.copy()
    bad = np.arange(5, d.shape[0], 97)
    d[bad[0::3], 0], d[bad[1::3], 1], d[bad[2::3], 2] = np.nan, np.inf, -np.inf
    m = d.shape[0]
    rays, hits, rows = np.zeros(2 * m, T.RAY32), np.zeros(2 * m, T.HIT32), np.zeros(2 * m, T.SURFACE64)
    rays["direction"][:m], rays["direction"][m:], rays["t_max"] = d, (0, 0, -1), FAR
    hits["prim_id"][:m], hits["prim_id"][m:], hits["t"][m:] = -1, 3, 2.0
    rng = np.random.default_rng(9)
    rows["normal"][m:], rows["n_dot_v"], rows["albedo"], rows["roughness"] = d, 0.5, rng.uniform(0.1, 0.9, (2 * m, 3)), 0.5
    rows["emission"][m:] = rng.uniform(0, 1, (m, 3))
    return rays, hits, rows, bad


def test_hand_placed_rays_and_non_finite_directions(built):
    rays, hits, rows, bad = placed_records()
    n, m = rays.shape[0], rays.shape[0] // 2
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        env = environment()
        d_rays, d_hits, d_rows, d_out = dev.put(rays), dev.put(hits), dev.put(rows), dev.alloc(n * 16)
        hit = hits["prim_id"] != -1
        with np.errstate(invalid="ignore"):
            p = rays["origin"] + rays["direction"] * hits["t"][:, None]
        for name in ("64x32", "3x2"):
            pano = (image(name), ENERGY)
            ctx.upload_panorama(*pano)
            ctx.light_surfaces(d_rays, d_hits, d_rows, n, light_list("soup")[:0], d_out, None, env)
            want = Lg.shade_linear(rows, hit, p, rays["direction"], [], None, env, panorama=pano)[0]
            got = dev.get(d_out, n * 4, F).reshape(-1, 4)
            np.testing.assert_array_equal(words(got), words(want))
            assert (words(got[bad]) == 0).all()                                     # a miss with a NaN direction: zeros
            np.testing.assert_array_equal(words(got[m + bad, :3]), words(rows["emission"][m + bad]))   # a hit with one: no ambient
            near = np.setdiff1d(np.concatenate([bad - 1, bad + 1]), bad)
            assert (got[near, :3] > 0).all() and (got[m + near, :3] > 0).all()       # their neighbours intact
    finally:
        dev.free()
        ctx.close()


def test_env_null_clear_replace_and_on_device(built):
    lit = Lit("soup", 100, 77)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        d = dev.alloc(n * 16)
        gradient, plain = lit.want(), lit.want(env=False)
        stats = ctx.stats()
        ctx.clear_panorama()                                                        # nothing resident: OK
        big, small = (image("257x129"), ENERGY), (image("3x2"), 0.5)
        ctx.upload_panorama(*big)
        assert ctx.stats() == stats                                                 # neither call touches mrt_stats
        lit.grid(d, env=False)
        check(dev, d, plain)
        lit.grid(d)
        check(dev, d, want_lit(lit, big))
        ctx.upload_panorama(*small)                                                 # another size replaces the first
        lit.grid(d)
        check(dev, d, want_lit(lit, small))
        ctx.upload_panorama(*big)                                                   # ... and growing again
        lit.grid(d)
        check(dev, d, want_lit(lit, big))
        d_img = dev.put(small[0])
        ctx.upload_panorama(d_img, small[1], on_device=True, size=(3, 2))
        lit.grid(d)
        check(dev, d, want_lit(lit, small))
        ctx.clear_panorama()
        lit.grid(d)
        check(dev, d, gradient)                                                     # the gradient again, byte for byte
        stats = ctx.stats()
        ctx.clear_panorama()
        assert ctx.stats() == stats
        # the scene is untouched: the same primary records
        d_hits = dev.alloc(n * 32)
        ctx.cast_grid(run.cam, run.w, run.h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        same(dev.get(d_hits, n, T.HIT32), run.hits)
    finally:
        lit.close()


def want_step(ch, pano, state, bounce, max_bounces, grid=True, info=None):
    r = ch.run
    pixel = ch.pixel if grid else np.arange(r.n, dtype=np.uint64)
    return P.path_step(state, ch.lit.rows, ch.lit.hit, ch.shits["normal"], r.rays["direction"], ch.direct, ch.env, pixel, FRAME, bounce,
                       max_bounces, info, panorama=pano)


@pytest.mark.parametrize("grid", [(100, 77, 0, 77), (128, 96, 20, 70)], ids=["100x77", "band"])
def test_path_steps_with_a_panorama(built, grid):
    """Bounce 0 from mrt_path_init's state and bounce 1 from a state in the middle of a path, grid and array forms: state, select and
    lobe bytes and the count."""
    ch = Chain("soup", *grid)
    run, lit = ch.run, ch.lit
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        pano = (image("64x32"), ENERGY)
        ctx.upload_panorama(*pano)
        d_rays = dev.put(run.rays)
        for bounce, state in ((0, P.init_state(n)), (1, mixed_state(n, 3))):
            info = {}
            want = want_step(ch, pano, state, bounce, 4, info=info)
            assert info["missed"].any() and want[3] > 0
            plain = ch.want(state, bounce, 4)
            assert (words(want[0]) != words(plain[0])).any() and np.array_equal(want[1], plain[1]) and np.array_equal(want[2], plain[2])
            o = Outputs(dev, n, state)
            ctx.path_grid_step(run.cam, run.w, run.h, ch.d_shits, lit.d_rows, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, bounce, 4,
                               o.d_lobe, o.d_count, y0=run.y0, y1=run.y1)
            o.check(want)
            o = Outputs(dev, n, state)
            ctx.path_step(d_rays, ch.d_shits, lit.d_rows, n, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, bounce, 4, o.d_lobe, o.d_count)
            o.check(want_step(ch, pano, state, bounce, 4, grid=False))
        ctx.clear_panorama()
        state = P.init_state(n)
        o = Outputs(dev, n, state)
        ctx.path_grid_step(run.cam, run.w, run.h, ch.d_shits, lit.d_rows, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, 0, 4,
                           o.d_lobe, o.d_count, y0=run.y0, y1=run.y1)
        o.check(ch.want(state, 0, 4))                                              # cleared: the gradient's step
    finally:
        ch.close()


def two_bounce_frame(ch, pano):
    """init, bounce 0 on the grid, the bounce cast, bounce 1 (the last) on its records, finish: the frame, and per pixel whether its
    path missed at either bounce"""
    run, lit = ch.run, ch.lit
    ctx, dev, n, w, h = run.ctx, run.dev, run.n, run.w, run.h
    if pano is None:
        ctx.clear_panorama()
    else:
        ctx.upload_panorama(*pano)
    lights = lit.lights[:4]
    shadow = capi.shadow_lights(lights)
    d_state, d_select, d_rgba = dev.alloc(n * 32), dev.alloc(n), dev.alloc(n * 16)
    d_rays1, d_hits1, d_rows1, d_shits1, d_mask1, d_direct1 = (dev.alloc(n * k) for k in (32, 32, 64, 32, 4, 16))
    ctx.path_init(d_state, n)
    ctx.path_grid_step(run.cam, w, h, ch.d_shits, lit.d_rows, ch.d_direct, d_state, ch.env, d_select, FRAME, 0, 1)
    ctx.cast_grid_bounce(run.cam, w, h, ch.d_shits, d_hits1, frame=FRAME, first_draw=P.first_draw(0), t_max=FAR, d_select=d_select,
                         d_surface=ch.d_pairs, d_out_rays=d_rays1)
    select0 = dev.get(d_select, n, np.uint8) != 0
    ctx.resolve_surfaces(d_rays1, d_hits1, n, d_rows1, d_out_hits=d_shits1)
    ctx.cast_shadows(d_rays1, d_hits1, n, shadow, d_mask1)
    ctx.light_surfaces(d_rays1, d_hits1, d_rows1, n, lights, d_direct1, d_mask1, None)
    ctx.path_step(d_rays1, d_shits1, d_rows1, n, d_direct1, d_state, ch.env, d_select, FRAME, 1, 1)
    ctx.path_finish(d_state, n, d_rgba, tonemap_mode=1)
    hit1 = dev.get(d_hits1, n, T.HIT32)["prim_id"] != -1
    return dev.get(d_rgba, n * 4, F).reshape(-1, 4), ~lit.hit, select0 & ~hit1


def test_a_two_bounce_frame_differs_only_where_a_path_missed(built):
    ch = Chain("soup", 100, 77)
    try:
        with_pano, miss0, miss1 = two_bounce_frame(ch, (image("64x32"), ENERGY))
        without, miss0b, miss1b = two_bounce_frame(ch, None)
        assert np.array_equal(miss0, miss0b) and np.array_equal(miss1, miss1b) and miss0.any() and miss1.any()
        differs = (words(with_pano) != words(without)).any(axis=1)
        missed = miss0 | miss1
        assert not differs[~missed].any()                                          # no miss on the path: the same pixel
        assert differs[miss0].all() and differs[miss1].any()                       # a primary miss shows the panorama itself
        assert np.isfinite(with_pano).all() and (with_pano[:, 3] == 1).all()
    finally:
        ch.close()


def test_refusals_and_pending(built):
    """Every refusal with and without a scene, before any device work: the resident panorama stays what it was."""
    L = capi.load()
    sc = scene("soup")
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        good = np.ascontiguousarray(image("3x2"))
        nan_img, inf_img = good.copy(), good.copy()
        nan_img[1, 2, 1], inf_img[0, 0, 2] = np.nan, -np.inf
        alpha_img = good.copy()
        alpha_img[..., 3] = np.nan                                                  # alpha is not read: accepted

        def up(img=good, w=3, h=2, energy=1.0, flags=0, null=False):
            d = capi.Panorama(None if null else img.ctypes.data, w, h, energy, flags)
            return L.mrt_upload_panorama(ctx.h, C.byref(d))

        def bad_calls():
            assert L.mrt_upload_panorama(ctx.h, None) == capi.ERR_INVALID
            for kw in (dict(null=True), dict(w=0), dict(h=0), dict(w=capi.PANORAMA_MAX_DIM + 1), dict(h=capi.PANORAMA_MAX_DIM + 1), dict(w=1 << 31),
                       dict(energy=np.nan), dict(energy=np.inf), dict(energy=-np.inf), dict(flags=2), dict(flags=3), dict(flags=1 << 31),
                       dict(img=nan_img), dict(img=inf_img)):
                assert up(**kw) == capi.ERR_INVALID, kw
                assert L.mrt_last_error(ctx.h) != b""

        rays = po.grid_rays(sc.cam[0], sc.cam[1], 64, 48, sc.cam[2])
        misses = np.zeros(64, T.HIT32)
        misses["prim_id"] = -1
        d_rays, d_hits, d_rows, d_out = dev.put(rays[:64]), dev.put(misses), dev.alloc(64 * 64), dev.alloc(64 * 16)
        env = environment()

        def sky():
            ctx.light_surfaces(d_rays, d_hits, d_rows, 64, light_list("soup")[:0], d_out, None, env)
            return dev.get(d_out, 64 * 4, F).reshape(-1, 4)[:, :3]

        gradient = sky()
        same(gradient, Lg.sky_gradient(rays["direction"][:64], env))
        bad_calls()                                                                 # no scene, nothing resident
        same(sky(), gradient)
        assert L.mrt_clear_panorama(ctx.h) == capi.MRT_OK
        assert up() == capi.MRT_OK and up(img=alpha_img) == capi.MRT_OK and up(energy=-2.0) == capi.MRT_OK and up(energy=2.0) == capi.MRT_OK
        resident = sky()
        same(resident, Pn.sky_panorama(good, 2.0, rays["direction"][:64]))
        bad_calls()                                                                 # the resident panorama is unchanged
        same(sky(), resident)
        sc.upload(ctx)
        upload(ctx, shade_data("soup"))
        bad_calls()
        same(sky(), resident)                                                       # it survives a scene upload
        ctx.submit(rays)
        assert up() == capi.ERR_PENDING and L.mrt_clear_panorama(ctx.h) == capi.ERR_PENDING
        assert up(w=0) == capi.ERR_INVALID                                          # the checks come before the pending test
        ctx.collect()
        same(sky(), resident)
        assert L.mrt_clear_panorama(ctx.h) == capi.MRT_OK and L.mrt_clear_panorama(ctx.h) == capi.MRT_OK
        same(sky(), gradient)
    finally:
        dev.free()
        ctx.close()


def test_primary_grid_unaffected_by_panorama_calls(built):
    """A renderer's frames: the primary grid with and without the panorama calls between frames -- the same kernels, the same records."""
    sc = scene("room")
    w, h = 320, 240
    lights = light_list("room")
    runs = []
    for with_pano in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            upload(ctx, shade_data("room"))
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits, d_rows, d_rgba = dev.alloc(w * h * 32), dev.alloc(w * h * 64), dev.alloc(w * h * 16)
            for f in range(6):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, w * h, T.HIT32).view(np.uint32))
                ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows)
                if with_pano:
                    if f % 3 == 0:
                        ctx.upload_panorama(image("64x32" if f else "3x2"), ENERGY)
                    if f == 4:
                        ctx.clear_panorama()
                ctx.light_grid_surfaces(cam, w, h, d_hits, d_rows, lights, d_rgba, None, environment(), flags=capi.FLAG_ASYNC if f & 1 else 0)
            runs.append((kernels, records))
        finally:
            dev.free()
            ctx.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)
