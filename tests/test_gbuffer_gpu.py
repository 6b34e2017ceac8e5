"""mrt_cast_gbuffer_reflections / mrt_reflection_image: the reflection effect's first pass from a rasteriser's depth and
normal-roughness buffers, against the formula restated in numpy float32 (messyerraytracer_amd/gbuffer.py; pinned to a second route and
to the host definitions by test_gbuffer_cpu.py) and traced by the oracle -- byte for byte.  The fixture (tests/gbuffer_cases.py) is
synth.room(), flat and two-level, seen through the helper's camera with a far plane: primary rays cast with mrt_cast, the hit points
projected to depths in float64, their normals octahedral-encoded, a roughness pattern that crosses the threshold.  67 x 35 (odd width,
a last partial wave) on the plain kernels and with the persistent ones forced, 256 x 257 on the persistent ones; the edge table's texels
scattered over the frame and poison in the normal texel of every sky pixel; MRT_NORMAL_WORLD and a singular projection; query masks; the
image with and without a lit buffer; the chain cast -> resolve -> shadows -> light -> image -> mrt_resolve_reflections against the same
chain of restatements; both calls ASYNC on a caller's stream behind the copy that writes the G-buffer; primary grids unaffected; errors."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import denoise as Dn
from messyerraytracer_amd import gbuffer as G
from messyerraytracer_amd import lighting as Lg
import gbuffer_cases as GC
from test_caller_stream_gpu import In, Out, Rig, miss_records, sequence
from test_hemisphere_gpu import Dev, hit_point, same, scene, shadow_mask
from test_lighting_gpu import environment, light_list
from test_surface_gpu import expected, shade_data, upload

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN = {"room": "trace_gbuffer_lane_kernel<13>", "room_tl": "trace_gbuffer_two_level_kernel<13>"}
PERSISTENT8 = {"room": "trace_gbuffer_persistent_kernel<13, 8, false>", "room_tl": "trace_gbuffer_persistent_kernel<13, 8, true>"}
FIXTURES, WANT = {}, {}


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fixture(kind, w, h):
    """The G-buffer of a frame, made once per scene kind and size: primary rays through the helper's camera cast with mrt_cast."""
    if (kind, w, h) not in FIXTURES:
        ctx = capi.Context(0)
        try:
            scene(kind).upload(ctx)
            fix = GC.Fixture(w, h, lambda rays: ctx.cast(rays))
        finally:
            ctx.close()
        same(fix.hits, scene(kind).oracle(fix.rays))
        print("[gbuffer] %s %d x %d: reconstructed positions within %.3f of their bound" % (kind, w, h, fix.position_error))
        FIXTURES[(kind, w, h)] = fix
    return FIXTURES[(kind, w, h)]


def frame(kind, w, h, edges=True, world=False, query_mask=0xFFFFFFFF):
    """(fixture, G.GBuffer, restated rays, traced, the oracle's records of them), made once; edges: the edge texels scattered over the
    frame and the sky's normal texels poisoned; world: the same frame as MRT_NORMAL_WORLD texels"""
    key = (kind, w, h, edges, world, query_mask)
    if key not in WANT:
        fix = fixture(kind, w, h)
        depth, guide = fix.depth.copy(), (fix.world_guide() if world else fix.guide.copy())
        if edges and not world:
            idx = GC.scatter_edges(fix, depth, guide)
        if edges:
            GC.poison_sky(depth, guide)
        g = fix.gbuffer(depth, guide, G.NORMAL_WORLD if world else G.NORMAL_OCTAHEDRAL)
        rays, traced = G.gbuffer_rays(g, w, h)
        want = scene(kind).oracle(rays, query_mask)
        if query_mask == 0xFFFFFFFF:
            fix.coverage(traced, want)
        if edges and not world:   # each edge texel decided as test_gbuffer_cpu.py says
            names = [GC.OCT_TEXELS[k % len(GC.OCT_TEXELS)][0] for k in range(idx.size)]
            off = {"depth exactly 1", "the float above 1", "a NaN depth", "the float above the threshold", "a NaN roughness", "a NaN normal texel",
                   "an infinite normal texel"}
            assert [bool(t) for t in traced[idx]] == [n not in off for n in names]
        same(want[~traced], np.repeat(G.PLACEHOLDER_HIT, (~traced).sum()))
        same(rays[~traced], np.repeat(G.PLACEHOLDER, (~traced).sum()))
        WANT[key] = (fix, g, rays, traced, want)
    return WANT[key]


class Frame:
    """a context with the scene resident and a frame's G-buffer on the device"""

    def __init__(self, kind, g, w, h, kernel=capi.KERNEL_AUTO):
        self.kind, self.g, self.w, self.h, self.n = kind, g, w, h, w * h
        self.ctx = capi.Context(0, kernel=kernel)
        self.dev = Dev(self.ctx)
        scene(kind).upload(self.ctx)
        self.d_depth, self.d_guide = self.dev.put(g.depth), self.dev.put(g.normal_roughness)
        self.desc = g.desc(self.d_depth, self.d_guide)

    def cast(self, query_mask=0xFFFFFFFF, flags=0, rays_out=True):
        d_hits, d_rays = self.dev.alloc(self.n * 32), (self.dev.alloc(self.n * 32) if rays_out else None)
        G.cast_gbuffer_reflections(self.ctx, self.desc, self.w, self.h, d_hits, d_rays, query_mask, flags)
        return d_hits, d_rays

    def close(self):
        self.dev.free()
        self.ctx.close()


def check_frame(kind, w, h, kernel, variant, **kw):
    fix, g, want_rays, traced, want = frame(kind, w, h, **kw)
    fr = Frame(kind, g, w, h, kernel)
    try:
        d_hits, d_rays = fr.cast()
        assert fr.ctx.last_kernel_variant() == variant, fr.ctx.last_kernel_variant()
        same(fr.dev.get(d_rays, fr.n, T.RAY32), want_rays)
        same(fr.dev.get(d_hits, fr.n, T.HIT32), want)
        # without d_out_rays: the same records
        d_hits2, _ = fr.cast(rays_out=False)
        same(fr.dev.get(d_hits2, fr.n, T.HIT32), want)
        # the inputs are only read
        same(fr.dev.get(fr.d_depth, fr.n, F), g.depth)
        same(fr.dev.get(fr.d_guide, fr.n * 4, F), g.normal_roughness.reshape(-1))
    finally:
        fr.close()


CASES = [(67, 35, capi.KERNEL_AUTO, PLAIN),
         (67, 35, capi.KERNEL_LANE_PERSISTENT, {"room": "trace_gbuffer_persistent_kernel<13, 2, false>", "room_tl": PLAIN["room_tl"]}),
         (67, 35, capi.KERNEL_LANE4_PERSISTENT, {"room": "trace_gbuffer_persistent_kernel<13, 4, false>", "room_tl": PLAIN["room_tl"]}),
         (67, 35, capi.KERNEL_LANE8_PERSISTENT, PERSISTENT8),
         (256, 257, capi.KERNEL_AUTO, PERSISTENT8)]


@pytest.mark.parametrize("kind", ["room", "room_tl"])
@pytest.mark.parametrize("case", CASES, ids=["67x35", "67x35-lane2p", "67x35-lane4p", "67x35-lane8p", "256x257"])
def test_frames_match_the_oracle(built, kind, case):
    """Rays and records of every pixel, the edge texels and the poisoned sky included, on every form of the family the policy can
    reach here.  (A two-level scene with 8-wide BLASes has one persistent form, the 8-wide one: a forced 2- or 4-wide persistent kernel
    gets the plain two-level kernel, as it does for a reflection cast.)"""
    w, h, kernel, variant = case
    check_frame(kind, w, h, kernel, variant[kind])


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_world_normals_and_a_singular_projection(built, kind):
    """The same frame as MRT_NORMAL_WORLD texels gives the same rays bit for bit (decode_guide's normal, handed over decoded); with
    row 3 of inv_projection zero q.3 is 0 everywhere and no pixel has a ray."""
    w, h = 67, 35
    check_frame(kind, w, h, capi.KERNEL_AUTO, PLAIN[kind], world=True)
    same(frame(kind, w, h, world=True)[2], frame(kind, w, h, edges=False)[2][:])
    fix, g, _, _, _ = frame(kind, w, h, edges=False)
    sing = g.inv_projection.copy()
    sing[3::4] = 0
    gs = fix.gbuffer(inv_projection=sing)
    rays, traced = G.gbuffer_rays(gs, w, h)
    assert not traced.any()
    fr = Frame(kind, gs, w, h)
    try:
        d_hits, d_rays = fr.cast()
        same(fr.dev.get(d_rays, fr.n, T.RAY32), np.repeat(G.PLACEHOLDER, fr.n))
        same(fr.dev.get(d_hits, fr.n, T.HIT32), np.repeat(G.PLACEHOLDER_HIT, fr.n))
    finally:
        fr.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_query_mask_leaves_the_walls_out(built, kind):
    w, h = 67, 35
    _, g, _, traced, want_all = frame(kind, w, h)
    _, _, _, _, want_obj = frame(kind, w, h, query_mask=1)
    assert (want_obj["prim_id"] != want_all["prim_id"]).any()   # the walls are on layer 2
    fr = Frame(kind, g, w, h)
    try:
        d_hits, _ = fr.cast(query_mask=1)
        same(fr.dev.get(d_hits, fr.n, T.HIT32), want_obj)
    finally:
        fr.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
@pytest.mark.parametrize("size", [(67, 35), (256, 257)], ids=["67x35", "256x257"])
def test_reflection_image(built, kind, size):
    """The image from the cast's records, without and with a lit buffer, against the restatement; guard words behind it."""
    w, h = size
    _, g, _, traced, want = frame(kind, w, h)
    n = w * h
    fr = Frame(kind, g, w, h)
    try:
        d_hits, _ = fr.cast()
        lit = np.random.default_rng(9).uniform(0, 3, (n, 4)).astype(F)
        d_lit = fr.dev.put(lit)
        guard = np.full(64, 0xA5A5A5A5, np.uint32)
        for dl, l in ((None, None), (d_lit, lit)):
            d_img = fr.dev.put(np.concatenate([np.full(n * 4, 0xA5A5A5A5, np.uint32), guard]))
            G.reflection_image_device(fr.ctx, fr.desc, w, h, d_hits, d_img, dl)
            got = fr.dev.get(d_img, n * 4 + 64, np.uint32)
            assert (got[n * 4:] == guard).all()
            want_img = G.reflection_image(g, w, h, want, l)
            np.testing.assert_array_equal(got[:n * 4], words(want_img).reshape(-1))
            hit = want["prim_id"] != -1
            assert (want_img[~hit] == 0).all() and (want_img[hit, 3] >= 0).all() and (want_img[hit, 3] <= 1).all() and hit.any()
        same(fr.dev.get(d_hits, n, T.HIT32), want)   # only read
    finally:
        fr.close()


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_chain_to_the_composite(built, kind):
    """A hybrid frame with nothing leaving the device: cast, mrt_resolve_surfaces, mrt_cast_shadows, mrt_light_surfaces,
    mrt_reflection_image(d_lit), mrt_resolve_reflections -- against the same chain of restatements."""
    w, h = 67, 35
    n = w * h
    _, g, want_rays, traced, want = frame(kind, w, h)
    sc = scene(kind)
    fr = Frame(kind, g, w, h)
    ctx, dev = fr.ctx, fr.dev
    try:
        shade = shade_data(kind)
        upload(ctx, shade)
        lights, env = light_list("room")[:4], environment()
        d_hits, d_rays = fr.cast()
        d_rows, d_mask, d_lit, d_img = dev.alloc(n * 64), dev.alloc(4 * n), dev.alloc(n * 16), dev.alloc(n * 16)
        ctx.resolve_surfaces(d_rays, d_hits, n, d_rows)
        ctx.cast_shadows(d_rays, d_hits, n, capi.shadow_lights(lights), d_mask)
        ctx.light_surfaces(d_rays, d_hits, d_rows, n, lights, d_lit, d_mask, env)
        G.reflection_image_device(ctx, fr.desc, w, h, d_hits, d_img, d_lit)
        rng = np.random.default_rng(21)
        color, hist = rng.uniform(0, 1, (h, w, 4)).astype(F), rng.uniform(0, 1, (h, w, 4)).astype(F)
        d_color, d_hist = dev.put(color), dev.put(hist)
        p = Dn.params(normal_kind=Dn.NORMAL_OCTAHEDRAL, has_history=True, roughness_threshold=float(GC.THRESHOLD), inv_view=g.inv_view)
        Dn.resolve_reflections(ctx, p, w, h, d_img, fr.d_depth, fr.d_guide, d_hist, d_color)
        # the same chain in numpy
        hit = want["prim_id"] != -1
        rows = expected(want_rays, want, shade)[0]
        mask = shadow_mask(sc, want_rays, want, capi.shadow_lights(lights))
        lit = Lg.shade_linear(rows, hit, hit_point(want_rays, want), want_rays["direction"], lights, mask.reshape(4, -1), env)[0]
        img = G.reflection_image(g, w, h, want, lit)
        # (poisoned sky texels: the spatial filter decodes every tap's normal, so the restatement sees what the device sees)
        _, want_hist, want_color = Dn.resolve(p, img.reshape(h, w, 4), g.depth.reshape(h, w), g.normal_roughness.reshape(h, w, 4), hist, color)
        same(dev.get(d_rows, n, T.SURFACE64), rows)
        np.testing.assert_array_equal(dev.get(d_mask, 4 * n, np.uint8), mask)
        np.testing.assert_array_equal(words(dev.get(d_lit, n * 4, F)), words(lit).reshape(-1))
        np.testing.assert_array_equal(words(dev.get(d_img, n * 4, F)), words(img).reshape(-1))
        for got, wanted, what in ((dev.get(d_hist, n * 4, F), want_hist, "history"), (dev.get(d_color, n * 4, F), want_color, "colour")):
            wanted = wanted.reshape(-1)
            nan = np.isnan(wanted)
            assert np.isnan(got[nan]).all(), what
            np.testing.assert_array_equal(words(got)[~nan], words(wanted)[~nan], err_msg=what)
        assert (mask == 0).any() and (words(want_color) != words(color)).any()   # shadows fell, reflections were blended in
    finally:
        fr.close()


def test_async_on_a_callers_stream(built):
    """Both calls queued with MRT_FLAG_ASYNC on a caller's stream behind the copies that write the G-buffer, the results copied out
    in stream order (the gated sequence of tests/test_caller_stream_gpu.py)."""
    kind, w, h = "room", 67, 35
    n = w * h
    _, g, want_rays, traced, want = frame(kind, w, h)
    want_img = G.reflection_image(g, w, h, want)
    rig = Rig(kind)
    try:
        # the decoy: a frame of sky
        depth = In(rig.dev, g.depth, np.ones(n, F))
        guide = In(rig.dev, g.normal_roughness, np.zeros((n, 4), F))
        desc = g.desc(depth.live, guide.live)
        hits, rays, img = Out(rig.dev, n * 32), Out(rig.dev, n * 32), Out(rig.dev, n * 16)

        def calls(flags):
            G.cast_gbuffer_reflections(rig.ctx, desc, w, h, hits.out, rays.out, flags=flags)
            G.reflection_image_device(rig.ctx, desc, w, h, hits.out, img.out, flags=flags)

        got, variant, _ = sequence(rig.ctx, rig.cs, [depth, guide], [hits, rays, img], calls, "gbuffer reflections")
        assert variant == PLAIN[kind]
        same(got[0].view(T.HIT32), want)
        same(got[1].view(T.RAY32), want_rays)
        np.testing.assert_array_equal(got[2].view(np.uint32), words(want_img).reshape(-1))
        assert not np.array_equal(want, miss_records(n))
    finally:
        rig.close()


def test_primary_grid_unaffected(built):
    """A primary mrt_cast_grid before and after a G-buffer cast and its image: identical records, the same variant label."""
    kind, w, h = "room", 256, 257
    _, g, _, _, _ = frame(kind, w, h)
    sc = scene(kind)
    fr = Frame(kind, g, w, h)
    try:
        cam = capi.camera_look(sc.cam[0], sc.cam[1], 640, 480, sc.cam[2])
        runs = []
        for k in range(4):
            runs.append((fr.ctx.cast_grid(cam, 640, 480).copy(), fr.ctx.stats()["last_kernel"], fr.ctx.last_kernel_variant()))
            if k >= 1:
                d_hits, _ = fr.cast()
                assert fr.ctx.last_kernel_variant() == PERSISTENT8[kind]
                G.reflection_image_device(fr.ctx, fr.desc, w, h, d_hits, fr.dev.alloc(fr.n * 16))
        # frames 0 -> 1 have no G-buffer cast between them, 1 -> 2 -> 3 do
        for a, b in zip(runs, runs[1:]):
            same(a[0], b[0])
        assert runs[0][2].startswith("trace_") and not any(r[2].startswith("trace_gbuffer") for r in runs)
        other = capi.Context(0)   # the same four grids with no G-buffer cast at all: the same labels, frame by frame
        try:
            sc.upload(other)
            for k in range(4):
                same(other.cast_grid(cam, 640, 480), runs[k][0])
                assert (other.stats()["last_kernel"], other.last_kernel_variant()) == runs[k][1:]
        finally:
            other.close()
    finally:
        fr.close()


def test_errors(built):
    """The error table of include/mrt_hip.h with a context: every refusal before any device work and in the documented order, nothing
    written; MRT_ERR_NO_SCENE; an empty frame; a pending dispatch."""
    L = G.lib()
    L.mrt_last_error.restype = C.c_char_p
    kind, w, h = "room", 67, 35
    n = w * h
    _, g, _, _, want = frame(kind, w, h)
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        d_depth, d_guide = dev.put(g.depth), dev.put(g.normal_roughness)
        pattern = np.full(n * 32, 7, np.uint8)
        d_out, d_img = dev.put(pattern), dev.put(pattern[:n * 16])
        V = C.c_void_p

        def desc(**kw):
            d = g.desc(kw.pop("d_depth", d_depth), kw.pop("d_guide", d_guide))
            for k, v in kw.items():
                if k in ("inv_projection", "inv_view"):
                    getattr(d, k)[v[0]] = v[1]
                else:
                    setattr(d, k, v)
            return d

        def cast(d="ok", ww=w, hh=h, out=d_out, flags=0):
            d = desc() if d == "ok" else d
            return L.mrt_cast_gbuffer_reflections(ctx.h, C.byref(d) if d is not None else None, ww, hh, V(out) if out else None, None, 0xFFFFFFFF, flags)

        def image(d="ok", ww=w, hh=h, hits=d_out, out=d_img, flags=0):
            d = desc() if d == "ok" else d
            return L.mrt_reflection_image(ctx.h, C.byref(d) if d is not None else None, ww, hh, V(hits) if hits else None, None,
                                          V(out) if out else None, flags)

        def refused(rc, word):
            return rc == capi.ERR_INVALID and word in L.mrt_last_error(ctx.h)

        nan, inf = float("nan"), float("inf")

        def bad_calls():
            for call in (cast, image):
                assert refused(call(d=None), b"null descriptor")
                assert refused(call(d=desc(d_depth=None)), b"null d_depth") and refused(call(d=desc(d_guide=None)), b"null d_normal_roughness")
                assert refused(call(d=desc(struct_size=156)), b"struct_size") and refused(call(d=desc(normal_kind=2)), b"normal_kind")
                assert refused(call(d=desc(inv_projection=(11, nan))), b"inv_projection") and refused(call(d=desc(inv_view=(3, inf))), b"inv_view")
                for t in (nan, inf, 0.0, -0.3):
                    assert refused(call(d=desc(roughness_threshold=t)), b"roughness_threshold")
                    assert refused(call(d=desc(max_distance=t)), b"max_distance")
                assert refused(call(ww=0xFFFFFFFF, hh=0xFFFFFFFF), b"overflows")
                for fl in (capi.FLAG_HOST_LAYOUT, capi.FLAG_BOOL_OUT, capi.FLAG_COHERENT, 1 << 20, capi.FLAG_ASYNC | capi.FLAG_TOKEN_OUT):
                    assert refused(call(flags=fl), b"flag")
            assert refused(cast(out=None), b"null d_out_hits")
            assert refused(image(hits=None), b"null d_hits") and refused(image(out=None), b"null d_reflection")
            # the order: wrong in everything, mended one at a time
            worst = desc(d_guide=None, struct_size=1, normal_kind=9, inv_view=(0, nan), roughness_threshold=-1.0, max_distance=nan)
            big = dict(ww=0xFFFFFFFF, hh=0xFFFFFFFF)
            assert refused(cast(d=worst, out=None, flags=1 << 20, **big), b"flag")            # the family's order: the flags first
            assert refused(cast(d=worst, out=None, **big), b"null d_normal_roughness")
            assert refused(image(d=worst, out=None, flags=1 << 20, **big), b"null d_reflection")
            assert refused(image(d=worst, flags=1 << 20, **big), b"flag")
            worst.d_normal_roughness = d_guide
            assert refused(cast(d=worst, out=None, **big), b"null d_out_hits")
            for call in (cast, image):
                w2 = desc(struct_size=1, normal_kind=9, inv_view=(0, nan), roughness_threshold=-1.0, max_distance=nan)
                assert refused(call(d=w2, **big), b"struct_size")
                w2.struct_size = 160
                assert refused(call(d=w2, **big), b"normal_kind")
                w2.normal_kind = 1
                assert refused(call(d=w2, **big), b"inv_view")
                w2.inv_view[0] = 1.0
                assert refused(call(d=w2, **big), b"roughness_threshold")
                w2.roughness_threshold = 0.3
                assert refused(call(d=w2, **big), b"max_distance")
                w2.max_distance = 4.0
                assert refused(call(d=w2, **big), b"overflows")

        bad_calls()   # before a scene is uploaded: the arguments are checked first
        assert cast() == capi.ERR_NO_SCENE and cast(ww=0) == capi.ERR_NO_SCENE
        assert image(ww=0) == capi.MRT_OK and image(hh=0) == capi.MRT_OK   # (the image reads no scene)
        scene(kind).upload(ctx)
        bad_calls()
        assert cast(ww=0) == capi.MRT_OK and cast(hh=0) == capi.MRT_OK and image(ww=0, hh=0) == capi.MRT_OK
        assert (dev.get(d_out, n * 32, np.uint8) == 7).all() and (dev.get(d_img, n * 16, np.uint8) == 7).all()   # no call so far wrote anything
        assert L.mrt_cast_gbuffer_reflections(None, C.byref(desc()), w, h, V(d_out), None, 0xFFFFFFFF, 0) == capi.ERR_INVALID
        assert L.mrt_reflection_image(None, C.byref(desc()), w, h, V(d_out), None, V(d_img), 0) == capi.ERR_INVALID
        # a pending dispatch
        rays = GC.camera(8, 8).primary_rays(8, 8)
        ctx.submit(rays)
        assert cast() == capi.ERR_PENDING and image() == capi.ERR_PENDING
        assert refused(cast(out=None), b"null d_out_hits")   # (the arguments still come first)
        ctx.collect()
        assert (dev.get(d_out, n * 32, np.uint8) == 7).all()
        assert cast() == capi.MRT_OK and image() == capi.MRT_OK
        same(dev.get(d_out, n, T.HIT32), want)
    finally:
        dev.free()
        ctx.close()
