"""mrt_cast_shadows / mrt_cast_grid_shadows: shadow rays made in the trace kernels from resident hit records, against the formula
restated in numpy float32 (messyerraytracer_amd/shadow.py, the way the oracle restates RayCamera) and traced by the oracle -- byte for byte -- and against the
same rays cast through mrt_cast(ANY_HIT, BOOL_OUT).  Flat and two-level synth.room(), a soup; grids with whole and clipped tiles and a
row band; one batch large enough for the persistent kernels; ASYNC; primary grids unaffected by shadow casts between them; errors."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from messyerraytracer_amd.shadow import shadow_rays
from oracle import pyoracle as po
import affine_scene

pytestmark = pytest.mark.gpu

F = np.float32
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
ROOM_CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
SOUP_CAM = ((0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0)


class Scene:
    def __init__(self, kind):
        self.kind = kind
        if kind == "soup":
            self.local, self.inst = synth.soup(2000, 0.4, 3), None
            self.verts, self.layers, self.cam = self.local, np.full(2000, 0xFFFFFFFF, np.uint32), SOUP_CAM
        elif kind == "affine_tl":   # mirrored, scaled and sheared instances, seen by their own camera (tests/affine_scene.py)
            a = affine_scene.scene()
            self.local, self.inst, self.verts, self.layers, self.cam = a.local, a.inst, a.world, a.layers, affine_scene.CAM
        else:
            self.local, self.inst = synth.room()
            self.verts = synth.flatten_instances(self.local, self.inst)
            self.layers = np.repeat(self.inst["layers"], self.inst["n_tris"]).astype(np.uint32)
            self.cam = ROOM_CAM
        self.two_level = kind.endswith("_tl")
        self._oracle = None

    def upload(self, ctx):
        if self.two_level:
            ctx.upload_two_level_scene(self.local, self.inst)
        else:
            tris = capi.make_triangles(self.verts, layers=self.layers)
            nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(self.verts))
            ctx.upload_scene(tris, nodes, prim_idx)

    def oracle_any(self, rays, query_mask=0xFFFFFFFF):
        if self._oracle is None:
            self._oracle = (po.OracleTwoLevelScene(self.local, self.inst) if self.two_level
                            else po.OracleScene(self.verts, layers=self.layers))
        return self._oracle.trace(rays, query_mask=query_mask, any_hit=True)["prim_id"] >= 0


SCENES = {}


def scene(kind):
    if kind not in SCENES:
        SCENES[kind] = Scene(kind)
    return SCENES[kind]


def light(kind, pos=(0, 0, 0), direction=(0, 0, 0), cast=1):
    L = np.zeros(1, dtype=T.LIGHT)
    L["type"], L["cast_shadows"], L["position"], L["direction"] = kind, cast, pos, direction
    return L


def lights_for(sc, org_of_a_hit):
    """Every kind of light in one call: directional, point, spot, one that casts no shadows, and a point light exactly on one
    pixel's shadow origin (dist == 0 < 1e-6: not traced)."""
    if sc.kind == "soup":
        ls = [light(T.LIGHT_DIRECTIONAL, direction=(0.2, 0.3, -1.0)), light(T.LIGHT_POINT, pos=(1.0, 0.5, -9.0)),
              light(T.LIGHT_SPOT, pos=(-3.0, 3.0, -7.0)), light(T.LIGHT_POINT, pos=(0.0, 0.0, -9.0), cast=0)]
    else:
        ls = [light(T.LIGHT_DIRECTIONAL, direction=(0.3, 1.0, 0.2)), light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5)),
              light(T.LIGHT_SPOT, pos=(-3.0, 5.0, -3.0)), light(T.LIGHT_POINT, pos=(0.0, 5.0, 0.0), cast=0)]
    ls.append(light(T.LIGHT_POINT, pos=org_of_a_hit))
    return np.concatenate(ls)


def expected(sc, pos, nrm, hit, lights, query_mask=0xFFFFFFFF):
    rays, traced = shadow_rays(pos, nrm, hit, lights)
    occluded = sc.oracle_any(rays, query_mask)
    assert not occluded[~traced].any()  # the degenerate rays of untraced pairs never report a hit
    return (~(traced & occluded)).astype(np.uint8), rays


class Dev:
    """device buffers of one context, freed at the end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.device_alloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def put(self, arr):
        p = self.alloc(arr.nbytes)
        self.ctx.h2d(p, arr)
        return p

    def get(self, p, n, dtype):
        out = np.zeros(n, dtype=dtype)
        self.ctx.d2h(out, p)
        return out

    def free(self):
        for p in self.ptrs:
            self.ctx.device_free(p)


def primary_grid(ctx, dev, sc, w, h, y0, y1, flags=0):
    origin, fwd, fov = sc.cam
    cam = capi.camera_look(origin, fwd, w, h, fov)
    n = w * (y1 - y0)
    d_hits = dev.alloc(n * 32)
    ctx.cast_grid(cam, w, h, y0=y0, y1=y1, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE | flags)
    return cam, d_hits, n


GRIDS = [(256, 192, 0, 192), (200, 77, 0, 77), (256, 192, 40, 150)]


def check_entry_points(kind, w, h, y0, y1, pick=None, kernel=capi.KERNEL_AUTO, variant="trace_shadow_"):
    """The three entry points on one grid of one scene, each mask against the oracle byte for byte, and the same rays through
    mrt_cast(ANY_HIT, BOOL_OUT).  pick: which of lights_for()'s five lights (all by default); variant: the prefix every shadow
    cast's kernel instantiation must have."""
    sc = scene(kind)
    ctx = capi.Context(0, kernel=kernel)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        cam, d_hits, n = primary_grid(ctx, dev, sc, w, h, y0, y1)
        hits = dev.get(d_hits, n, T.HIT32)
        rays = po.grid_rays(sc.cam[0], sc.cam[1], w, h, sc.cam[2], y0, y1)
        hit = hits["prim_id"] != -1
        assert hit.any()
        pos = rays["origin"] + rays["direction"] * hits["t"][:, None]
        first = int(np.flatnonzero(hit)[0])
        lights = lights_for(sc, pos[first] + hits["normal"][first] * F(1e-3))
        if pick is None:
            want, srays = expected(sc, pos, hits["normal"], hit, lights)
            assert want.min() == 0 and want.max() == 1
            assert want[(len(lights) - 1) * n + first] == 1  # the light on that pixel's shadow origin: not traced, lit
        else:
            lights = lights[list(pick)]
            want, srays = expected(sc, pos, hits["normal"], hit, lights)

        # (1) the grid: primary rays regenerated in the kernel
        d_mask = dev.alloc(n * len(lights))
        ctx.cast_grid_shadows(cam, w, h, d_hits, lights, d_mask, y0=y0, y1=y1)
        assert ctx.last_kernel_variant().startswith(variant), ctx.last_kernel_variant()
        np.testing.assert_array_equal(dev.get(d_mask, n * len(lights), np.uint8), want)

        # (2) 32-byte records written by mrt_cast for the same rays
        d_rays, d_h32 = dev.put(rays), dev.alloc(n * 32)
        ctx.cast(d_rays, d_h32, count=n, flags=DEV)
        d_mask2 = dev.alloc(n * len(lights))
        ctx.cast_shadows(d_rays, d_h32, n, lights, d_mask2)
        assert ctx.last_kernel_variant().startswith(variant), ctx.last_kernel_variant()
        np.testing.assert_array_equal(dev.get(d_mask2, n * len(lights), np.uint8), want)

        # (3) the reference's host layout: Ray / Intersection records
        hrays = po.make_host_rays(rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        want44, _ = expected(sc, h44["position"], h44["normal"], h44["prim_id"] != T.NO_HIT, lights)
        np.testing.assert_array_equal(want44, want)  # the record's position is o + d * t too
        d_mask3 = dev.alloc(n * len(lights))
        ctx.cast_shadows(d_hr, d_h44, n, lights, d_mask3, flags=capi.FLAG_HOST_LAYOUT)
        assert ctx.last_kernel_variant().startswith(variant), ctx.last_kernel_variant()
        np.testing.assert_array_equal(dev.get(d_mask3, n * len(lights), np.uint8), want)

        # (4) the same rays cast through mrt_cast(ANY_HIT, BOOL_OUT)
        occ = ctx.cast(srays, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        np.testing.assert_array_equal((1 - occ).astype(np.uint8), want)
    finally:
        dev.free()
        ctx.close()


@pytest.mark.parametrize("kind", ["room", "room_tl", "soup"])
@pytest.mark.parametrize("grid", GRIDS, ids=["256x192", "200x77", "band"])
def test_shadow_masks_match_the_oracle(built, kind, grid):
    check_entry_points(kind, *grid)   # (5 lights: 77 000 - 245 760 pairs, the persistent kernels)


PLAIN = {"room": "trace_shadow_lane_kernel<", "room_tl": "trace_shadow_two_level_kernel<", "affine_tl": "trace_shadow_two_level_kernel<"}


# Below 2^16 pairs the plain kernels: 64x48 with one light is 3 072 pairs (one ray per wave), with five 15 360 (two per wave), 256x192
# with one light 49 152 (full waves); the row band: 200 x 30 rows, one light.
@pytest.mark.parametrize("kind", ["room", "room_tl"])
@pytest.mark.parametrize("case", [((64, 48, 0, 48), (1,)), ((64, 48, 0, 48), None), ((256, 192, 0, 192), (1,)),
                                  ((200, 77, 20, 50), (2,))], ids=["64x48-1", "64x48-5", "256x192-1", "band-1"])
def test_small_batches_run_the_plain_kernels(built, kind, case):
    grid, pick = case
    check_entry_points(kind, *grid, pick=pick, variant=PLAIN[kind])


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_forced_lane_kernel_on_a_large_batch(built, kind):
    """MRT_KERNEL_LANE forced: 2^21 pairs (1024 x 1024, two lights) in the plain kernel, full waves."""
    check_entry_points(kind, 1024, 1024, 0, 1024, pick=(1, 2), kernel=capi.KERNEL_LANE, variant=PLAIN[kind])


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_query_mask_leaves_the_walls_out(built, kind):
    sc = scene(kind)
    w, h = 256, 192
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        cam, d_hits, n = primary_grid(ctx, dev, sc, w, h, 0, h)
        hits = dev.get(d_hits, n, T.HIT32)
        rays = po.grid_rays(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
        hit = hits["prim_id"] != -1
        pos = rays["origin"] + rays["direction"] * hits["t"][:, None]
        lights = np.concatenate([light(T.LIGHT_DIRECTIONAL, direction=(0.3, 1.0, 0.2)), light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5))])
        want_all, _ = expected(sc, pos, hits["normal"], hit, lights)
        want_obj, _ = expected(sc, pos, hits["normal"], hit, lights, query_mask=1)
        assert (want_obj == 0).any()
        assert (want_obj != want_all).any()  # the ceiling shadows everything from the directional light, the objects do not
        d_mask = dev.alloc(2 * n)
        ctx.cast_grid_shadows(cam, w, h, d_hits, lights, d_mask, query_mask=1)
        np.testing.assert_array_equal(dev.get(d_mask, 2 * n, np.uint8), want_obj)
    finally:
        dev.free()
        ctx.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_large_batch_runs_the_persistent_kernels(built, kind):
    sc = scene(kind)
    w = h = 1024
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        cam, d_hits, n = primary_grid(ctx, dev, sc, w, h, 0, h)
        hits = dev.get(d_hits, n, T.HIT32)
        rays = po.grid_rays(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
        pos = rays["origin"] + rays["direction"] * hits["t"][:, None]
        lights = np.concatenate([light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5)), light(T.LIGHT_SPOT, pos=(-3.0, 5.0, -3.0))])
        want, _ = expected(sc, pos, hits["normal"], hits["prim_id"] != -1, lights)
        d_mask = dev.alloc(2 * n)
        ctx.cast_grid_shadows(cam, w, h, d_hits, lights, d_mask)
        persistent = (capi.KERNEL_LANE_PERSISTENT, capi.KERNEL_LANE4_PERSISTENT, capi.KERNEL_LANE8_PERSISTENT,
                      capi.KERNEL_TWO_LEVEL_PERSISTENT, capi.KERNEL_TWO_LEVEL_PERSISTENT8)
        assert ctx.stats()["last_kernel"] in persistent
        assert "shadow_persistent" in ctx.last_kernel_variant()
        np.testing.assert_array_equal(dev.get(d_mask, 2 * n, np.uint8), want)
        # flat scene: forced 2- and 4-wide persistent kernels; both: a forced packet kernel (which gives the policy's lane kernel)
        forced = (capi.KERNEL_LANE_PERSISTENT, capi.KERNEL_LANE4_PERSISTENT, capi.KERNEL_PACKET_ASM) if kind == "room" else (capi.KERNEL_PACKET_ASM,)
        for k in forced:
            c2 = capi.Context(0, kernel=k)
            d2 = Dev(c2)
            try:
                sc.upload(c2)
                dh, dm = d2.put(hits), d2.alloc(2 * n)
                c2.cast_grid_shadows(cam, w, h, dh, lights, dm)
                assert c2.stats()["last_kernel"] in persistent
                np.testing.assert_array_equal(d2.get(dm, 2 * n, np.uint8), want)
            finally:
                d2.free()
                c2.close()
    finally:
        dev.free()
        ctx.close()


def test_async_grid_then_async_shadows(built):
    sc = scene("room")
    w, h = 320, 240
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        lights = np.concatenate([light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5)), light(T.LIGHT_DIRECTIONAL, direction=(0.3, 1.0, 0.2))])
        cam, d_hits, n = primary_grid(ctx, dev, sc, w, h, 0, h)
        d_mask = dev.alloc(2 * n)
        ctx.cast_grid_shadows(cam, w, h, d_hits, lights, d_mask)
        blocking = dev.get(d_mask, 2 * n, np.uint8)
        d_hits2, d_mask2 = dev.alloc(n * 32), dev.alloc(2 * n)
        ctx.cast_grid(cam, w, h, hits=d_hits2, flags=capi.FLAG_HITS_ON_DEVICE | capi.FLAG_ASYNC)
        ctx.cast_grid_shadows(cam, w, h, d_hits2, lights, d_mask2, flags=capi.FLAG_ASYNC)
        ctx.synchronize()
        np.testing.assert_array_equal(dev.get(d_mask2, 2 * n, np.uint8), blocking)
        np.testing.assert_array_equal(dev.get(d_hits2, n, T.HIT32).view(np.uint32), dev.get(d_hits, n, T.HIT32).view(np.uint32))
    finally:
        dev.free()
        ctx.close()


def test_primary_grid_unaffected_by_shadow_casts(built):
    """A renderer's frames: the primary grid (scheduled from the second frame on: 2^17 rays and more) with and without shadow casts
    between frames -- the same kernel sequence, the same records."""
    sc = scene("room")
    w, h = 640, 480
    runs = []
    for shadows in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            lights = np.concatenate([light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5))])
            kernels, records = [], []
            d_mask = dev.alloc(w * h)
            for f in range(14):
                cam, d_hits, n = primary_grid(ctx, dev, sc, w, h, 0, h)
                kernels.append(ctx.stats()["last_kernel"])
                records.append(dev.get(d_hits, n, T.HIT32).view(np.uint32))
                if shadows:
                    ctx.cast_grid_shadows(cam, w, h, d_hits, lights, d_mask)
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
        lights = np.concatenate([light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5))] * 2)
        lp = lights.ctypes.data_as(C.c_void_p)
        cam = capi.camera_look(sc.cam[0], sc.cam[1], 64, 48, sc.cam[2])
        d_rays, d_hits, d_mask = dev.alloc(64 * 48 * 32), dev.alloc(64 * 48 * 32), dev.alloc(2 * 64 * 48)
        R, H, M = C.c_void_p(d_rays), C.c_void_p(d_hits), C.c_void_p(d_mask)

        def shadows(rays=R, hits=H, count=64, lights_=lp, n=2, mask=M, flags=0):
            return L.mrt_cast_shadows(ctx.h, rays, hits, count, lights_, n, mask, 0xFFFFFFFF, flags)

        def grid(hits=H, lights_=lp, n=2, mask=M, flags=0, camera=cam):
            return L.mrt_cast_grid_shadows(ctx.h, C.byref(camera) if camera is not None else None, 64, 48, 0, 48, hits, lights_, n,
                                           mask, 0xFFFFFFFF, flags)

        assert shadows() == capi.ERR_NO_SCENE and grid() == capi.ERR_NO_SCENE  # before a scene is uploaded
        sc.upload(ctx)
        ctx.cast_grid(cam, 64, 48, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        assert shadows() == capi.MRT_OK and grid() == capi.MRT_OK
        many = np.concatenate([lights] * 9)
        assert shadows(lights_=many.ctypes.data_as(C.c_void_p), n=17) == capi.ERR_INVALID   # > MRT_MAX_LIGHTS
        assert grid(lights_=many.ctypes.data_as(C.c_void_p), n=17) == capi.ERR_INVALID
        for kw in (dict(rays=None), dict(hits=None), dict(mask=None), dict(lights_=None)):
            assert shadows(**kw) == capi.ERR_INVALID, kw
        for kw in (dict(hits=None), dict(mask=None), dict(lights_=None), dict(camera=None)):
            assert grid(**kw) == capi.ERR_INVALID, kw
        assert shadows(count=(1 << 63) + 1) == capi.ERR_INVALID                            # count * n_lights overflows
        bad = lights.copy()
        bad["type"][1] = 3
        assert shadows(lights_=bad.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID         # unknown light type
        assert grid(lights_=bad.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID
        for f in (capi.FLAG_BOOL_OUT, capi.FLAG_COHERENT, capi.FLAG_TOKEN_OUT, 1 << 20):
            assert shadows(flags=f) == capi.ERR_INVALID and grid(flags=f) == capi.ERR_INVALID, f
        assert grid(flags=capi.FLAG_HOST_LAYOUT) == capi.ERR_INVALID                       # grid records are mrt_hit32
        # no lights: MRT_OK, nothing written
        ctx.h2d(d_mask, np.full(2 * 64 * 48, 7, np.uint8))
        assert shadows(n=0, lights_=None) == capi.MRT_OK and grid(n=0, lights_=None) == capi.MRT_OK
        assert (dev.get(d_mask, 2 * 64 * 48, np.uint8) == 7).all()
        assert L.mrt_cast_shadows(None, R, H, 64, lp, 2, M, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    finally:
        dev.free()
        ctx.close()
