"""mrt_cast_reflections / mrt_cast_grid_reflections: mirror-reflection rays made in the trace kernels from resident hit records,
against the formula restated in numpy float32 (messyerraytracer_amd/reflection.py, one operation at a time) and traced by the oracle -- byte for byte -- and against
the same rays cast through mrt_cast(NEAREST).  A soup (back faces: the normal flip), flat and two-level synth.room(); grids with whole
and clipped tiles and a row band, records of mrt_cast in both layouts; the rays written out; selection masks; query masks; the plain
and the persistent kernels; chained shadow casts and a second bounce; ASYNC; primary grids unaffected; errors."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from messyerraytracer_amd import reflection as R
from messyerraytracer_amd import shadow as S
from oracle import pyoracle as po
import affine_scene

pytestmark = pytest.mark.gpu

F = np.float32
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
ROOM_CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
SOUP_CAM = ((0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0)
MAX_DIST = F(25.0)
PLACEHOLDER, PLACEHOLDER_HIT = R.PLACEHOLDER, R.PLACEHOLDER_HIT  # the reference's Ray(0, (0, 1, 0), 0, 0) and mrt_cast's record of it


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

    def oracle(self, rays, query_mask=0xFFFFFFFF, any_hit=False):
        if self._oracle is None:
            self._oracle = (po.OracleTwoLevelScene(self.local, self.inst) if self.two_level
                            else po.OracleScene(self.verts, layers=self.layers))
        return self._oracle.trace(rays, query_mask=query_mask, any_hit=any_hit)


SCENES = {}


def scene(kind):
    if kind not in SCENES:
        SCENES[kind] = Scene(kind)
    return SCENES[kind]


def reflection_rays(dirs, pos, nrm, traced, max_distance=MAX_DIST):
    """messyerraytracer_amd/reflection.py at this file's max_distance"""
    return R.reflection_rays(dirs, pos, nrm, traced, max_distance)


def hit_point(rays, hits):
    with np.errstate(over="ignore", invalid="ignore"):
        return rays["origin"] + rays["direction"] * hits["t"][:, None]


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


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
        self.ctx.h2d(p, np.ascontiguousarray(arr))
        return p

    def get(self, p, n, dtype):
        out = np.zeros(n, dtype=dtype)
        self.ctx.d2h(out, p)
        return out

    def free(self):
        for p in self.ptrs:
            self.ctx.device_free(p)


class Run:
    """one context with the scene uploaded and the primary grid of rows [y0, y1) cast into device records"""

    def __init__(self, kind, w, h, y0=0, y1=None, kernel=capi.KERNEL_AUTO):
        self.sc, self.w, self.h, self.y0, self.y1 = scene(kind), w, h, y0, h if y1 is None else y1
        self.ctx = capi.Context(0, kernel=kernel)
        self.dev = Dev(self.ctx)
        self.sc.upload(self.ctx)
        origin, fwd, fov = self.sc.cam
        self.cam = capi.camera_look(origin, fwd, w, h, fov)
        self.n = w * (self.y1 - self.y0)
        self.rays = po.grid_rays(origin, fwd, w, h, fov, self.y0, self.y1)
        self.d_hits = self.dev.alloc(self.n * 32)
        self.ctx.cast_grid(self.cam, w, h, y0=self.y0, y1=self.y1, hits=self.d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        self.hits = self.dev.get(self.d_hits, self.n, T.HIT32)
        assert (self.hits["prim_id"] != -1).any()

    def close(self):
        self.dev.free()
        self.ctx.close()

    def grid_reflections(self, select=None, query_mask=0xFFFFFFFF, flags=0):
        """mrt_cast_grid_reflections: (records, rays) read back"""
        d_sel = self.dev.put(select.astype(np.uint8)) if select is not None else None
        d_out, d_orays = self.dev.alloc(self.n * 32), self.dev.alloc(self.n * 32)
        self.ctx.cast_grid_reflections(self.cam, self.w, self.h, self.d_hits, d_out, MAX_DIST, d_select=d_sel, d_out_rays=d_orays,
                                       y0=self.y0, y1=self.y1, query_mask=query_mask, flags=flags)
        return d_out, d_orays

    def expected(self, select=None, query_mask=0xFFFFFFFF):
        traced = self.hits["prim_id"] != -1
        if select is not None:
            traced &= select != 0
        rays, flipped = reflection_rays(self.rays["direction"], hit_point(self.rays, self.hits), self.hits["normal"], traced)
        return rays, self.sc.oracle(rays, query_mask), traced, flipped


def check_all_entry_points(kind, w, h, y0=0, y1=None, kernel=capi.KERNEL_AUTO, variant=None):
    """The grid form and the ray form in both layouts on one grid of one scene: records and rays against the restated formula traced
    by the oracle, byte for byte, and against mrt_cast(NEAREST) of the restated rays.  variant: the kernel every cast must report."""
    run = Run(kind, w, h, y0, y1, kernel)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        want_rays, want, traced, flipped = run.expected()
        assert traced.any()
        if kind == "soup":  # (the room is closed: every primary ray hits)
            assert (~traced).any() and flipped.any()  # back faces: the normal was turned towards the incoming ray
        assert (want["prim_id"][traced] != -1).any()
        same(want[~traced], np.repeat(PLACEHOLDER_HIT, (~traced).sum()))

        # (1) the grid: incoming rays regenerated in the kernel
        d_out, d_orays = run.grid_reflections()
        if variant:
            assert ctx.last_kernel_variant().startswith(variant), ctx.last_kernel_variant()
        same(dev.get(d_out, n, T.HIT32), want)
        same(dev.get(d_orays, n, T.RAY32), want_rays)

        # (2) 32-byte records written by mrt_cast for the same rays
        d_rays, d_h32 = dev.put(run.rays), dev.alloc(n * 32)
        ctx.cast(d_rays, d_h32, count=n, flags=DEV)
        d_out2, d_orays2 = dev.alloc(n * 32), dev.alloc(n * 32)
        ctx.cast_reflections(d_rays, d_h32, n, d_out2, MAX_DIST, d_out_rays=d_orays2)
        if variant:
            assert ctx.last_kernel_variant().startswith(variant.replace("<6", "<4")), ctx.last_kernel_variant()
        same(dev.get(d_out2, n, T.HIT32), want)
        same(dev.get(d_orays2, n, T.RAY32), want_rays)

        # (3) the reference's host layout: Ray / Intersection records in, Ray / Intersection out
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        traced44 = h44["prim_id"] != T.NO_HIT
        want_rays44, _ = reflection_rays(hrays["direction"], h44["position"], h44["normal"], traced44)
        same(want_rays44, want_rays)  # the record's position is o + d * t too
        d_out3, d_orays3 = dev.alloc(n * 44), dev.alloc(n * 60)
        ctx.cast_reflections(d_hr, d_h44, n, d_out3, MAX_DIST, d_out_rays=d_orays3, flags=capi.FLAG_HOST_LAYOUT)
        if variant:
            assert ctx.last_kernel_variant().startswith(variant.replace("<6", "<5")), ctx.last_kernel_variant()
        host_want_rays = po.make_host_rays(want_rays)
        same(dev.get(d_out3, n, T.HOST_HIT44), po.unpack_hits(want, host_want_rays))
        same(dev.get(d_orays3, n, T.HOST_RAY60), host_want_rays)

        # (4) the same rays uploaded and cast through mrt_cast(NEAREST)
        d_rr, d_hr2 = dev.put(want_rays), dev.alloc(n * 32)
        ctx.cast(d_rr, d_hr2, count=n, flags=DEV)
        same(dev.get(d_hr2, n, T.HIT32), want)
    finally:
        run.close()


GRIDS = [(128, 96, 0, 96), (100, 77, 0, 77), (128, 96, 20, 70)]
PLAIN = {"room": "trace_reflection_lane_kernel<6>", "room_tl": "trace_reflection_two_level_kernel<6>",
         "soup": "trace_reflection_lane_kernel<6>", "affine_tl": "trace_reflection_two_level_kernel<6>"}


@pytest.mark.parametrize("kind", ["soup", "room", "room_tl"])
@pytest.mark.parametrize("grid", GRIDS, ids=["128x96", "100x77", "band"])
def test_reflections_match_the_oracle(built, kind, grid):
    check_all_entry_points(kind, *grid, variant=PLAIN[kind])   # (below 2^16 records: the plain kernels)


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_large_batch_runs_the_persistent_kernels(built, kind):
    """256 x 256 = 2^16 records: the persistent kernels (8-wide; two-level: 8-wide BLASes), every source."""
    check_all_entry_points(kind, 256, 256, variant="trace_reflection_persistent_kernel<6, 8, %s>" % ("true" if kind == "room_tl" else "false"))


@pytest.mark.parametrize("kernel, variant", [(capi.KERNEL_LANE, "trace_reflection_lane_kernel<6>"),
                                             (capi.KERNEL_LANE4_PERSISTENT, "trace_reflection_persistent_kernel<6, 4, false>"),
                                             (capi.KERNEL_LANE8_PERSISTENT, "trace_reflection_persistent_kernel<6, 8, false>"),
                                             (capi.KERNEL_PACKET_ASM, "trace_reflection_persistent_kernel<6, ")],
                         ids=["lane", "lane4p", "lane8p", "packet"])
def test_forced_kernels(built, kernel, variant):
    """A forced kernel on a 2^16-record grid; a forced packet kernel means the policy's lane kernel (persistent, of the width the
    context's scene layouts allow)."""
    check_all_entry_points("room", 256, 256, kernel=kernel, variant=variant)


def test_forced_lane_kernel_two_level(built):
    check_all_entry_points("room_tl", 256, 256, kernel=capi.KERNEL_LANE, variant="trace_reflection_two_level_kernel<6>")


@pytest.mark.parametrize("kind", ["room", "room_tl"])
@pytest.mark.parametrize("size", [(128, 96), (256, 256)], ids=["plain", "persistent"])
def test_selection_masks(built, kind, size):
    """A seeded random mask and an all-zero one: unselected records and primary misses hold the placeholder's record and ray."""
    w, h = size
    run = Run(kind, w, h)
    try:
        rng = np.random.default_rng(7)
        for sel in (rng.random(run.n) < 0.4, np.zeros(run.n, dtype=bool)):
            want_rays, want, traced, _ = run.expected(select=sel)
            d_out, d_orays = run.grid_reflections(select=sel)
            same(run.dev.get(d_out, run.n, T.HIT32), want)
            same(run.dev.get(d_orays, run.n, T.RAY32), want_rays)
            same(want[~traced], np.repeat(PLACEHOLDER_HIT, (~traced).sum()))
            # the ray form in the host layout with the same mask
            hrays = po.make_host_rays(run.rays)
            d_hr, d_h44 = run.dev.put(hrays), run.dev.alloc(run.n * 44)
            run.ctx.cast(d_hr, d_h44, count=run.n, flags=DEV | capi.FLAG_HOST_LAYOUT)
            d_out3 = run.dev.alloc(run.n * 44)
            run.ctx.cast_reflections(d_hr, d_h44, run.n, d_out3, MAX_DIST, d_select=run.dev.put(sel.astype(np.uint8)),
                                     flags=capi.FLAG_HOST_LAYOUT)
            same(run.dev.get(d_out3, run.n, T.HOST_HIT44), po.unpack_hits(want, po.make_host_rays(want_rays)))
        assert not traced.any()
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_query_mask_leaves_the_walls_out(built, kind):
    run = Run(kind, 128, 96)
    try:
        _, want_all, _, _ = run.expected()
        _, want_obj, traced, _ = run.expected(query_mask=1)
        assert (want_obj["prim_id"] != want_all["prim_id"]).any()   # the walls (layer 2) mirror each other; masked, they do not
        d_out, _ = run.grid_reflections(query_mask=1)
        same(run.dev.get(d_out, run.n, T.HIT32), want_obj)
    finally:
        run.close()


def shadow_mask(sc, rays, hits, lights):
    """The shadow formula of include/mrt_hip.h (messyerraytracer_amd/shadow.py) traced by the oracle: 1 lit, 0 shadowed, light-major."""
    srays, traced = S.shadow_rays(hit_point(rays, hits), hits["normal"], hits["prim_id"] != -1, lights)
    occ = sc.oracle(srays, any_hit=True)["prim_id"] >= 0
    return (~(traced & occ)).astype(np.uint8)


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_chained_shadows_and_second_bounce(built, kind):
    run = Run(kind, 160, 120)
    ctx, dev, n, sc = run.ctx, run.dev, run.n, run.sc
    try:
        rays1, hits1, _, _ = run.expected()
        d_out, d_orays = run.grid_reflections()
        same(dev.get(d_out, n, T.HIT32), hits1)
        # shadows at the reflected points
        lights = np.zeros(2, dtype=T.LIGHT)
        lights["cast_shadows"] = 1
        lights[0]["type"], lights[0]["position"] = T.LIGHT_POINT, (1.0, 4.5, 1.5)
        lights[1]["type"], lights[1]["direction"] = T.LIGHT_DIRECTIONAL, (0.3, 1.0, 0.2)
        want_mask = shadow_mask(sc, rays1, hits1, lights)
        assert want_mask.min() == 0 and want_mask.max() == 1
        d_mask = dev.alloc(2 * n)
        ctx.cast_shadows(d_orays, d_out, n, lights, d_mask)
        np.testing.assert_array_equal(dev.get(d_mask, 2 * n, np.uint8), want_mask)
        # a second mirror bounce from the first one's outputs
        traced2 = hits1["prim_id"] != -1
        rays2, _ = reflection_rays(rays1["direction"], hit_point(rays1, hits1), hits1["normal"], traced2)
        hits2 = sc.oracle(rays2)
        assert (hits2["prim_id"] != -1).any()
        d_out2, d_orays2 = dev.alloc(n * 32), dev.alloc(n * 32)
        ctx.cast_reflections(d_orays, d_out, n, d_out2, MAX_DIST, d_out_rays=d_orays2)
        same(dev.get(d_out2, n, T.HIT32), hits2)
        same(dev.get(d_orays2, n, T.RAY32), rays2)
        # the same chain in the host layout: Ray / Intersection out of the first bounce into the shadow cast and the second bounce
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        d_o44, d_or60 = dev.alloc(n * 44), dev.alloc(n * 60)
        ctx.cast_reflections(d_hr, d_h44, n, d_o44, MAX_DIST, d_out_rays=d_or60, flags=capi.FLAG_HOST_LAYOUT)
        d_mask44 = dev.alloc(2 * n)
        ctx.cast_shadows(d_or60, d_o44, n, lights, d_mask44, flags=capi.FLAG_HOST_LAYOUT)
        np.testing.assert_array_equal(dev.get(d_mask44, 2 * n, np.uint8), want_mask)
        d_o44b = dev.alloc(n * 44)
        ctx.cast_reflections(d_or60, d_o44, n, d_o44b, MAX_DIST, flags=capi.FLAG_HOST_LAYOUT)
        same(dev.get(d_o44b, n, T.HOST_HIT44), po.unpack_hits(hits2, po.make_host_rays(rays2)))
    finally:
        run.close()


def test_async_grid_then_async_reflections(built):
    run = Run("room", 160, 120)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        _, want, _, _ = run.expected()
        d_hits2, d_out = dev.alloc(n * 32), dev.alloc(n * 32)
        ctx.cast_grid(run.cam, run.w, run.h, hits=d_hits2, flags=capi.FLAG_HITS_ON_DEVICE | capi.FLAG_ASYNC)
        ctx.cast_grid_reflections(run.cam, run.w, run.h, d_hits2, d_out, MAX_DIST, flags=capi.FLAG_ASYNC)
        d_rays, d_out2 = dev.put(run.rays), dev.alloc(n * 32)
        ctx.cast_reflections(d_rays, d_hits2, n, d_out2, MAX_DIST, flags=capi.FLAG_ASYNC)
        ctx.synchronize()
        same(dev.get(d_out, n, T.HIT32), want)
        same(dev.get(d_out2, n, T.HIT32), want)
    finally:
        run.close()


def test_primary_grid_unaffected_by_reflection_casts(built):
    """A renderer's frames: the primary grid (scheduled from the second frame on: 2^17 rays and more) with and without reflection
    casts between frames -- the same kernel sequence, the same records."""
    sc = scene("room")
    w, h = 640, 480
    runs = []
    for reflections in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits, d_out = dev.alloc(w * h * 32), dev.alloc(w * h * 32)
            for f in range(14):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, w * h, T.HIT32).view(np.uint32))
                if reflections:
                    ctx.cast_grid_reflections(cam, w, h, d_hits, d_out, MAX_DIST)
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
        d_rays, d_hits, d_out = dev.alloc(n * 60), dev.alloc(n * 44), dev.alloc(n * 44)
        R, H, O = C.c_void_p(d_rays), C.c_void_p(d_hits), C.c_void_p(d_out)
        pattern = np.full(n * 44, 7, np.uint8)
        ctx.h2d(d_out, pattern)

        def refl(rays=R, hits=H, count=n, out=O, dist=10.0, flags=0):
            return L.mrt_cast_reflections(ctx.h, rays, hits, count, None, dist, out, None, 0xFFFFFFFF, flags)

        def grid(hits=H, out=O, dist=10.0, flags=0, camera=cam, y0=0, y1=h):
            return L.mrt_cast_grid_reflections(ctx.h, C.byref(camera) if camera is not None else None, w, h, y0, y1, hits, None, dist,
                                               out, None, 0xFFFFFFFF, flags)

        def bad_calls():
            for kw in (dict(rays=None), dict(hits=None), dict(out=None), dict(dist=float("nan")), dict(dist=float("inf")),
                       dict(dist=0.0), dict(dist=-1.0)):
                assert refl(**kw) == capi.ERR_INVALID, kw
            for kw in (dict(hits=None), dict(out=None), dict(camera=None), dict(dist=float("nan")), dict(dist=-float("inf")),
                       dict(dist=0.0), dict(y0=10, y1=5), dict(y1=h + 1), dict(flags=capi.FLAG_HOST_LAYOUT)):
                assert grid(**kw) == capi.ERR_INVALID, kw
            for f in (capi.FLAG_BOOL_OUT, capi.FLAG_TOKEN_OUT, capi.FLAG_COHERENT, capi.FLAG_FORCE_SORT, 1 << 20):
                assert refl(flags=f) == capi.ERR_INVALID and grid(flags=f) == capi.ERR_INVALID, f

        bad_calls()   # before a scene is uploaded: the arguments are checked first
        assert refl() == capi.ERR_NO_SCENE and grid() == capi.ERR_NO_SCENE
        assert refl(count=0) == capi.ERR_NO_SCENE
        sc.upload(ctx)
        bad_calls()
        assert refl(count=0) == capi.MRT_OK  # nothing to do
        assert (dev.get(d_out, n * 44, np.uint8) == 7).all()  # no call so far wrote anything
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        assert grid() == capi.MRT_OK and grid(y0=10, y1=10) == capi.MRT_OK
        assert L.mrt_cast_reflections(None, R, H, n, None, 10.0, O, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
        assert L.mrt_cast_grid_reflections(None, C.byref(cam), w, h, 0, h, H, None, 10.0, O, None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    finally:
        dev.free()
        ctx.close()
