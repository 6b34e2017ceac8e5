"""mrt_light_surfaces / mrt_light_grid_surfaces: Cook-Torrance direct light over all lights (and, with an environment, the sky, ambient
and emission terms of shade_material) on resolved surfaces, held to the numpy restatement (messyerraytracer_amd/lighting.py; pinned to
the reference by test_lighting_cpu.py) as uint32 words, byte for byte.  The scenes, grids and shade data of test_surface_gpu.py; one
seeded list of sixteen lights per scene in which, among the hits of every grid, a light beyond its range, a surface outside a cone,
inside one with a fractional falloff, facing away, shadowed by the mask mrt_cast_grid_shadows wrote and lit by a light that casts no
shadows all occur.  Grid, array and host-layout forms; with and without the mask and the environment; 0, 1 and 16 lights; 1, 255, 257
and 2^16 + 1 records; a band; ASYNC; nothing resident; the chain on bounce records; guards; refusals; primary grids unaffected."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import surface as S
from oracle import pyoracle as po
from test_hemisphere_gpu import DEV, Dev, Run, hit_point, same, scene
from test_surface_gpu import GRIDS, GRID_IDS, KINDS, expected, shade_data, upload, words

pytestmark = pytest.mark.gpu

F = np.float32
FAR = F(1e30)
LIGHTS = {}


def light_list(kind):
    """Sixteen seeded lights of a scene, made once.  The first six are placed by hand (a sun, a light from below that most surfaces
    face away from and that casts no shadows, a point light that reaches everything, one of short range, a narrow spot with a
    fractional falloff, a wide one that casts no shadows); the rest are drawn."""
    if kind not in LIGHTS:
        rng = np.random.default_rng(4160 + len(kind))
        room = kind != "soup"
        centre = np.array([0, 2.5, -1] if room else [0, 0, 0], np.float64)
        reach = 4.0 if room else 3.0
        ls = np.zeros(16, T.SHADE_LIGHT)
        ls["cast_shadows"], ls["range"], ls["attenuation"], ls["spot_angle"], ls["spot_angle_attenuation"] = 1, 10, 1, 0.785398, 1
        ls["direction"], ls["color"] = (0, 1, 0), rng.uniform(0.2, 3.0, size=(16, 3))
        ls["type"][:6] = (0, 0, 1, 1, 2, 2)
        ls["direction"][0] = (0.3, 1.0, 0.2) if room else (0.3, 0.4, -1.0)
        ls["direction"][1], ls["cast_shadows"][1] = ((0, -1, 0) if room else (0, 0, 1)), 0
        ls["position"][2], ls["range"][2] = centre + (1.0, 2.0, 1.5 if room else -4.0), 40
        ls["position"][3], ls["range"][3], ls["attenuation"][3] = centre + (reach * 0.7, -1.5, -1.0), 2.5, 2
        ls["position"][4], ls["direction"][4] = centre + ((0, 3.2, 0) if room else (0, 0, -6)), ((0, 1, 0) if room else (0, 0, -1))
        ls["spot_angle"][4], ls["spot_angle_attenuation"][4], ls["range"][4] = 0.5, 0.5, 30
        ls["position"][5], ls["direction"][5] = centre + ((-3, 2.5, 2) if room else (-3, 2, -5)), ((-0.6, 0.6, 0.5) if room else (-0.5, 0.3, -0.8))
        ls["spot_angle"][5], ls["spot_angle_attenuation"][5], ls["range"][5], ls["cast_shadows"][5], ls["attenuation"][5] = 1.1, 2, 25, 0, 0.5
        for l in range(6, 16):
            t = int(rng.integers(0, 3))
            ls["type"][l] = t
            pos = centre + rng.uniform(-reach, reach, 3) * ((1, 0.6, 1) if room else (1, 1, 1))
            ls["position"][l] = pos
            axis = pos - (centre + rng.uniform(-2, 2, 3))                     # from a point of the scene towards the light
            ls["direction"][l] = axis / np.linalg.norm(axis) if t != 0 else rng.normal(size=3)
            ls["range"][l] = rng.uniform(2.0, 14.0)
            ls["attenuation"][l] = rng.choice([1, 2, 0.5, 0, 3.7])
            ls["spot_angle"][l] = rng.uniform(0.3, 1.3)
            ls["spot_angle_attenuation"][l] = rng.choice([1, 2, 0.5, 0.8])
            ls["cast_shadows"][l] = rng.random() < 0.7
        LIGHTS[kind] = ls
    return LIGHTS[kind]


def environment():
    env = np.zeros(1, T.ENVIRONMENT)
    env["sky_zenith"], env["sky_horizon"], env["sky_ground"] = (0.15, 0.25, 0.55), (0.6, 0.7, 0.85), (0.15, 0.12, 0.1)
    env["ambient"], env["ambient_energy"] = (1.0, 0.9, 0.8), 0.15
    return env[0]


def assert_cases_occur(kind, rows, hit, p, lights, mask):
    """Among the hits: beyond range, outside a cone, inside one with a fractional falloff, facing away, shadowed, lit by a light that
    casts no shadows -- each in a pair the other skips do not already drop (float64 geometry: this only counts)."""
    n = rows["normal"][hit].astype(np.float64)
    pp = p[hit].astype(np.float64)
    m = mask.reshape(lights.shape[0], -1)[:, hit]
    seen = dict(beyond=False, outside=False, fractional=False, away=False, shadowed=False, unshadowed=False)
    for l, L in enumerate(lights):
        ok = np.ones(pp.shape[0], bool)
        if L["type"] == T.LIGHT_DIRECTIONAL:
            Lv = np.tile(L["direction"].astype(np.float64), (pp.shape[0], 1))
        else:
            to = L["position"].astype(np.float64) - pp
            dist = np.linalg.norm(to, axis=1)
            seen["beyond"] |= bool((dist > L["range"]).any())
            ok &= (dist <= L["range"]) & (dist > 1e-6)
            Lv = to / dist[:, None]
            if L["type"] == T.LIGHT_SPOT:
                co = np.cos(np.float64(L["spot_angle"]))
                ca = Lv @ L["direction"].astype(np.float64)
                seen["outside"] |= bool((ok & (ca < co - 1e-4)).any())
                t = (ca - co) / (1 - co)
                seen["fractional"] |= bool((ok & (t > 0.05) & (t < 0.95) & (L["spot_angle_attenuation"] != 0)).any())
                ok &= ca > co + 1e-4
        ndl = (n * Lv).sum(axis=1)
        seen["away"] |= bool((ok & (ndl < -1e-3)).any())
        ok &= ndl > 1e-3
        seen["shadowed"] |= bool((ok & (m[l] == 0)).any()) and bool(L["cast_shadows"])
        seen["unshadowed"] |= bool(ok.any()) and not L["cast_shadows"] and bool((m[l] == 1).all())
    assert all(seen.values()), (kind, seen)


class Lit:
    """A Run with shade data resident (or none), its rows resolved, the mask of the scene's lights cast, all on the device and the host."""

    def __init__(self, kind, w, h, y0=0, y1=None, shade=True):
        self.run = run = Run(kind, w, h, y0, y1)
        ctx, dev, n = run.ctx, run.dev, run.n
        self.kind, self.lights = kind, light_list(kind)
        self.shade = shade_data(kind) if shade else None
        if shade:
            upload(ctx, self.shade)
        self.d_rows = dev.alloc(n * 64)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, run.d_hits, self.d_rows, y0=run.y0, y1=run.y1)
        self.rows = dev.get(self.d_rows, n, T.SURFACE64)
        self.d_mask = dev.alloc(16 * n)
        ctx.cast_grid_shadows(run.cam, run.w, run.h, run.d_hits, capi.shadow_lights(self.lights), self.d_mask, y0=run.y0, y1=run.y1)
        self.mask = dev.get(self.d_mask, 16 * n, np.uint8)
        self.hit = run.hits["prim_id"] != -1
        self.p = hit_point(run.rays, run.hits)
        self.env = environment()

    def want(self, n_lights=16, mask=True, env=True):
        m = self.mask.reshape(16, -1)[:n_lights] if mask else None
        return Lg.shade_linear(self.rows, self.hit, self.p, self.run.rays["direction"], self.lights[:n_lights], m, self.env if env else None)[0]

    def grid(self, d_rgba, n_lights=16, mask=True, env=True, flags=0):
        r = self.run
        r.ctx.light_grid_surfaces(r.cam, r.w, r.h, r.d_hits, self.d_rows, self.lights[:n_lights], d_rgba, self.d_mask if mask else None,
                                  self.env if env else None, y0=r.y0, y1=r.y1, flags=flags)

    def close(self):
        self.run.close()


def check(dev, d_rgba, want):
    got = dev.get(d_rgba, want.shape[0] * 4, F).reshape(-1, 4)
    np.testing.assert_array_equal(words(got), words(want))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_every_form_matches_the_restatement(built, kind, grid):
    """Grid form, array form and host-layout array form, with the mask and the environment; the grid form also without either and
    with 0 and 1 lights."""
    lit = Lit(kind, *grid)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        np.testing.assert_array_equal(words(lit.rows), words(expected(run.rays, run.hits, lit.shade)[0]))
        assert_cases_occur(kind, lit.rows, lit.hit, lit.p, lit.lights, lit.mask)
        want = lit.want()
        assert np.isfinite(want).all() and (want[lit.hit, :3] > 0).any() and (want[lit.hit, 3] == 1).all() and (want[~lit.hit, 3] == 0).all()
        d_rgba = dev.alloc(n * 16)
        lit.grid(d_rgba)
        check(dev, d_rgba, want)
        for kw in (dict(mask=False), dict(env=False), dict(mask=False, env=False), dict(n_lights=0), dict(n_lights=0, env=False),
                   dict(n_lights=1), dict(n_lights=1, mask=False, env=False)):
            other = lit.want(**kw)
            lit.grid(d_rgba, **kw)
            check(dev, d_rgba, other)
        assert (words(lit.want(mask=False)) != words(want)).any() and (words(lit.want(env=False)) != words(want)).any()
        assert (lit.want(n_lights=0, env=False) == np.where(lit.hit[:, None], F([0, 0, 0, 1]), F(0))).all()
        # the array form on what mrt_cast read and wrote (the mask is indexed [l * count + i]: the band's own)
        d_rays = dev.put(run.rays)
        d_out = dev.alloc(n * 16)
        ctx.light_surfaces(d_rays, run.d_hits, lit.d_rows, n, lit.lights, d_out, lit.d_mask, lit.env)
        check(dev, d_out, want)
        # the reference's host layout
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        d_rows44, d_mask44, d_out44 = dev.alloc(n * 64), dev.alloc(16 * n), dev.alloc(n * 16)
        ctx.resolve_surfaces(d_hr, d_h44, n, d_rows44, flags=capi.FLAG_HOST_LAYOUT)
        ctx.cast_shadows(d_hr, d_h44, n, capi.shadow_lights(lit.lights), d_mask44, flags=capi.FLAG_HOST_LAYOUT)
        rows44, mask44 = dev.get(d_rows44, n, T.SURFACE64), dev.get(d_mask44, 16 * n, np.uint8)
        want44 = Lg.shade_linear(rows44, h44["prim_id"] != T.NO_HIT, h44["position"], hrays["direction"], lit.lights, mask44.reshape(16, -1), lit.env)[0]
        ctx.light_surfaces(d_hr, d_h44, d_rows44, n, lit.lights, d_out44, d_mask44, lit.env, flags=capi.FLAG_HOST_LAYOUT)
        check(dev, d_out44, want44)
    finally:
        lit.close()


@pytest.mark.parametrize("count", [1, 255, 257, 2 ** 16 + 1])
def test_array_counts_and_guards(built, count):
    """The array form on the first `count` records of a 257 x 256 grid: one record, one short of a workgroup, one past it, one past
    2^16; the floats behind the output and the buffers beside it keep their pattern."""
    lit = Lit("soup", 257, 256)
    run = lit.run
    ctx, dev = run.ctx, run.dev
    try:
        d_rays = dev.put(run.rays)
        d_mask = dev.alloc(16 * count)
        ctx.cast_shadows(d_rays, run.d_hits, count, capi.shadow_lights(lit.lights), d_mask)
        mask = dev.get(d_mask, 16 * count, np.uint8).reshape(16, count)
        assert lit.hit[:count].any() or count == 1
        want = Lg.shade_linear(lit.rows[:count], lit.hit[:count], lit.p[:count], run.rays["direction"][:count], lit.lights, mask, lit.env)[0]
        guard = np.full((count + 64) * 4, -7.5, F)
        d_before, d_out, d_after = dev.put(guard[:256]), dev.put(guard), dev.put(guard[:256])
        before = [dev.get(p, k, np.uint8) for p, k in ((lit.d_rows, run.n * 64), (run.d_hits, run.n * 32), (d_rays, run.n * 32), (d_mask, 16 * count))]
        ctx.light_surfaces(d_rays, run.d_hits, lit.d_rows, count, lit.lights, d_out, d_mask, lit.env)
        got = dev.get(d_out, (count + 64) * 4, F)
        np.testing.assert_array_equal(words(got[:count * 4].reshape(-1, 4)), words(want))
        assert (got[count * 4:] == F(-7.5)).all() and (dev.get(d_before, 256, F) == F(-7.5)).all() and (dev.get(d_after, 256, F) == F(-7.5)).all()
        after = [dev.get(p, k, np.uint8) for p, k in ((lit.d_rows, run.n * 64), (run.d_hits, run.n * 32), (d_rays, run.n * 32), (d_mask, 16 * count))]
        for a, b in zip(before, after):
            np.testing.assert_array_equal(a, b)                                 # the inputs are read only
    finally:
        lit.close()


def test_a_band_lights_what_the_whole_frame_lights(built):
    whole, band = Lit("room", 128, 96), Lit("room", 128, 96, 20, 70)
    try:
        outs = []
        for lit in (whole, band):
            d = lit.run.dev.alloc(lit.run.n * 16)
            lit.grid(d)
            outs.append(lit.run.dev.get(d, lit.run.n * 4, F).reshape(-1, 4))
        same(outs[0][20 * 128:70 * 128], outs[1])
    finally:
        whole.close()
        band.close()


def test_async_then_synchronize(built):
    lit = Lit("soup", 100, 77)
    run = lit.run
    try:
        d_rays = run.dev.put(run.rays)
        a, b = run.dev.alloc(run.n * 16), run.dev.alloc(run.n * 16)
        lit.grid(a, flags=capi.FLAG_ASYNC)
        run.ctx.light_surfaces(d_rays, run.d_hits, lit.d_rows, run.n, lit.lights, b, lit.d_mask, lit.env, flags=capi.FLAG_ASYNC)
        run.ctx.synchronize()
        check(run.dev, a, lit.want())
        check(run.dev, b, lit.want())
    finally:
        lit.close()


@pytest.mark.parametrize("kind", ["soup", "room_tl"])
def test_rows_resolved_with_nothing_resident(built, kind):
    """The default material and the face normal everywhere: no emission, the same call."""
    lit = Lit(kind, 100, 77, shade=False)
    try:
        assert (lit.rows["material"] == T.DEFAULT_MATERIAL).all() and (lit.rows["emission"] == 0).all()
        d = lit.run.dev.alloc(lit.run.n * 16)
        for kw in (dict(), dict(env=False, mask=False)):
            lit.grid(d, **kw)
            check(lit.run.dev, d, lit.want(**kw))
    finally:
        lit.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_chain_on_bounce_records(built, kind):
    """cast -> bounce -> shadows -> resolve -> light, all on the records and rays mrt_cast_grid_bounce wrote: next-event estimation at
    a path's second vertex."""
    lit = Lit(kind, 96, 72)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        d_pairs = dev.alloc(n * 8)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, run.d_hits, d_bounce_surface=d_pairs)
        d_hits1, d_rays1 = dev.alloc(n * 32), dev.alloc(n * 32)
        ctx.cast_grid_bounce(run.cam, run.w, run.h, run.d_hits, d_hits1, frame=3, t_max=FAR, d_surface=d_pairs, d_out_rays=d_rays1)
        rays1, hits1 = dev.get(d_rays1, n, T.RAY32), dev.get(d_hits1, n, T.HIT32)
        hit1 = hits1["prim_id"] != -1
        assert hit1.any() and (~hit1).any()                                     # (records without a ray are misses of the placeholder)
        d_mask1, d_rows1, d_out = dev.alloc(16 * n), dev.alloc(n * 64), dev.alloc(n * 16)
        ctx.cast_shadows(d_rays1, d_hits1, n, capi.shadow_lights(lit.lights), d_mask1)
        ctx.resolve_surfaces(d_rays1, d_hits1, n, d_rows1)
        ctx.light_surfaces(d_rays1, d_hits1, d_rows1, n, lit.lights, d_out, d_mask1, lit.env)
        rows1, mask1 = dev.get(d_rows1, n, T.SURFACE64), dev.get(d_mask1, 16 * n, np.uint8)
        np.testing.assert_array_equal(words(rows1), words(expected(rays1, hits1, lit.shade)[0]))
        want = Lg.shade_linear(rows1, hit1, hit_point(rays1, hits1), rays1["direction"], lit.lights, mask1.reshape(16, -1), lit.env)[0]
        assert (want[hit1, :3] > 0).any() and (mask1 == 0).any()
        check(dev, d_out, want)
    finally:
        lit.close()


def test_refusals_count_zero_and_pending(built):
    """Every refusal, with and without a scene, before anything is written; count == 0 is OK and writes nothing; no scene is needed."""
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
        rows = expected(rays, hits, None)[0]
        lights = light_list("soup")
        env = np.zeros(1, T.ENVIRONMENT)
        env[0] = environment()
        mask = np.ones(16 * n, np.uint8)
        mask[::3] = 0
        d_rays, d_hits, d_rows, d_mask = dev.put(rays), dev.put(hits), dev.put(rows), dev.put(mask)
        pattern = np.full(n * 4, -7.5, F)
        d_out = dev.put(pattern)
        R, Hp, Rw, M = (C.c_void_p(x) for x in (d_rays, d_hits, d_rows, d_mask))
        good_out = capi.LightOut(d_out)

        def ptr(a):
            return None if a is None else a.ctypes.data_as(C.c_void_p)

        def arr(rays=R, hits=Hp, rows=Rw, count=n, ls=lights, n_lights=16, m=M, e=env, out=good_out, flags=0):
            return L.mrt_light_surfaces(ctx.h, rays, hits, rows, count, ptr(ls), n_lights, m, ptr(e), None if out is None else C.byref(out), flags)

        def grid(hits=Hp, rows=Rw, ls=lights, n_lights=16, m=M, e=env, out=good_out, flags=0, camera=cam, y0=0, y1=h):
            return L.mrt_light_grid_surfaces(ctx.h, None if camera is None else C.byref(camera), w, h, y0, y1, hits, rows, ptr(ls), n_lights, m,
                                             ptr(e), None if out is None else C.byref(out), flags)

        def changed(**fields):
            ls = lights.copy()
            for k, v in fields.items():
                ls[k][9] = v
            return ls

        def bad_env(word):
            e = env.copy()
            e.view(F)[word] = np.inf
            return e

        def bad_calls():
            many = np.concatenate([lights, lights[:1]])
            common = [dict(hits=None), dict(rows=None), dict(out=None), dict(out=capi.LightOut(None)), dict(ls=None), dict(ls=many, n_lights=17),
                      dict(ls=changed(type=3)), dict(ls=changed(reserved=1)), dict(ls=changed(color=(1, np.nan, 1))), dict(ls=changed(position=(np.inf, 0, 0))),
                      dict(ls=changed(direction=(0, 0, -np.inf))), dict(ls=changed(spot_angle=np.nan)), dict(ls=changed(type=1, range=0)),
                      dict(ls=changed(type=2, range=-1)), dict(ls=changed(type=1, range=np.inf)), dict(ls=changed(attenuation=-0.5)),
                      dict(ls=changed(spot_angle_attenuation=-1)), dict(e=bad_env(0)), dict(e=bad_env(12)), dict(e=bad_env(7), n_lights=0)]
            for kw in common + [dict(rays=None), dict(count=(1 << 64) // 16 + 1)]:
                assert arr(**kw) == capi.ERR_INVALID, kw
            for kw in common + [dict(camera=None), dict(y0=10, y1=5), dict(y1=h + 1), dict(flags=capi.FLAG_HOST_LAYOUT)]:
                assert grid(**kw) == capi.ERR_INVALID, kw
            for fl in (capi.FLAG_BOOL_OUT, capi.FLAG_TOKEN_OUT, capi.FLAG_COHERENT, capi.FLAG_FORCE_SORT, capi.FLAG_RAYS_ON_DEVICE, 1 << 20):
                assert arr(flags=fl) == capi.ERR_INVALID and grid(flags=fl) == capi.ERR_INVALID, fl
            assert arr(ls=changed(type=0, range=0)) == capi.MRT_OK                 # a directional light's range is not looked at
            ctx.h2d(d_out, pattern)

        def untouched():
            return (dev.get(d_out, n * 4, F) == F(-7.5)).all()

        bad_calls()                                   # no scene
        assert arr(count=0) == capi.MRT_OK and grid(y0=10, y1=10) == capi.MRT_OK and arr(count=0, ls=None, n_lights=0) == capi.MRT_OK
        assert untouched()
        hit, p = hits["prim_id"] != -1, hit_point(rays, hits)
        want = Lg.shade_linear(rows, hit, p, rays["direction"], lights, mask.reshape(16, -1), env[0])[0]
        assert grid() == capi.MRT_OK                  # no scene is required
        check(dev, d_out, want)
        assert arr(ls=None, n_lights=0, m=None, e=None) == capi.MRT_OK
        check(dev, d_out, Lg.shade_linear(rows, hit, p, rays["direction"], lights[:0], None, None)[0])
        sc.upload(ctx)
        upload(ctx, shade_data("soup"))
        bad_calls()
        assert untouched()
        ctx.submit(rays)
        assert arr() == capi.ERR_PENDING and grid() == capi.ERR_PENDING
        assert arr(ls=changed(type=3)) == capi.ERR_INVALID                       # the checks come before the pending test
        ctx.collect()
        assert untouched()
        assert arr() == capi.MRT_OK
        check(dev, d_out, want)
    finally:
        dev.free()
        ctx.close()


def test_primary_grid_unaffected_by_lighting_calls(built):
    """A renderer's frames: the primary grid with and without the lit chain between frames -- the same kernel sequence, the same records."""
    sc = scene("room")
    w, h = 640, 480
    lights = light_list("room")
    runs = []
    for lighting in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            upload(ctx, shade_data("room"))
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits, d_rows, d_mask, d_rgba = dev.alloc(w * h * 32), dev.alloc(w * h * 64), dev.alloc(w * h * 16), dev.alloc(w * h * 16)
            ctx.h2d(d_mask, np.ones(w * h * 16, np.uint8))
            for f in range(8):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, w * h, T.HIT32).view(np.uint32))
                if lighting:
                    ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows)
                    ctx.light_grid_surfaces(cam, w, h, d_hits, d_rows, lights, d_rgba, d_mask, environment(), flags=capi.FLAG_ASYNC if f & 1 else 0)
            runs.append((kernels, records))
        finally:
            dev.free()
            ctx.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)
