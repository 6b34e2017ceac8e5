"""The reflection effect's image passes on the device (mrt_denoise_spatial, mrt_denoise_temporal, mrt_composite_reflections,
mrt_resolve_reflections, mrt_reflection_guides), held to the numpy float32 restatement (messyerraytracer_amd/denoise.py; pinned to a
float64 evaluation and to the host definitions by test_denoise_cpu.py) word for word, a NaN for a NaN.  Image sizes around the 16 x 16
tile and smaller than the halo, both normal kinds, every radius; hand-made edge inputs; every temporal branch at its threshold; the
composite's clamps; the fused call against the three in sequence over three frames; the guides of a cast; one reflected frame end to
end; ASYNC, refusals, a pending dispatch and primary grids unaffected.  Guard words behind every output."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import denoise as Dn
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import reflection as R
from oracle import pyoracle as po
from test_denoise_cpu import images, rotation
from test_hemisphere_gpu import Dev, hit_point, same, scene
from test_lighting_gpu import environment, light_list
from test_surface_gpu import expected, shade_data, upload

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
PATTERN = 0xA5A5A5A5
SIZES = [(1, 1), (1, 9), (9, 1), (3, 2), (15, 15), (16, 16), (17, 17), (33, 17), (64, 48)]
KINDS = (Dn.NORMAL_OCTAHEDRAL, Dn.NORMAL_WORLD)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_floats(got, want, what=""):
    """bit for bit, but a NaN for a NaN whatever its payload"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what
    np.testing.assert_array_equal(words(got)[~nan], words(want)[~nan], err_msg=what)


class Img:
    """an image on the device, guard words behind it"""

    def __init__(self, dev, arr=None, shape=None):
        self.dev = dev
        self.shape = shape if arr is None else np.shape(arr)
        n = int(np.prod(self.shape))
        first = np.full(n, PATTERN, np.uint32) if arr is None else words(np.ascontiguousarray(arr, dtype=F)).reshape(-1)
        self.n, self.p = n, dev.put(np.concatenate([first, np.full(GUARD, PATTERN, np.uint32)]))

    def read(self):
        got = self.dev.get(self.p, self.n + GUARD, np.uint32)
        assert (got[self.n:] == PATTERN).all(), "guard words overwritten"
        return got[:self.n].view(F).reshape(self.shape)

    def untouched(self):
        return (self.dev.get(self.p, self.n + GUARD, np.uint32) == PATTERN).all()


@pytest.fixture(scope="module")
def gpu(built):
    ctx = capi.Context(0)
    dev = Dev(ctx)
    yield ctx, dev
    dev.free()
    ctx.close()


def release(dev):
    dev.free()
    dev.ptrs.clear()


def run_all(ctx, dev, p, refl, depth, guide, hist, color, what):
    """the three calls in sequence and the fused call against the restatement; returns the restated (denoised, history, colour)"""
    h, w = depth.shape
    d_refl, d_depth, d_guide = Img(dev, refl), Img(dev, depth), Img(dev, guide)
    want_den, want_hist, want_color = Dn.resolve(p, refl, depth, guide, hist, color)
    d_den, d_hist, d_color = Img(dev, shape=(h, w, 4)), Img(dev, hist), Img(dev, color)
    Dn.denoise_spatial(ctx, p, w, h, d_refl.p, d_depth.p, d_guide.p, d_den.p)
    same_floats(d_den.read(), want_den, what + ": spatial")
    Dn.denoise_temporal(ctx, p, w, h, d_den.p, d_hist.p, d_hist.p)
    same_floats(d_hist.read(), want_hist, what + ": temporal")
    Dn.composite_reflections(ctx, p, w, h, d_hist.p, d_depth.p, d_guide.p, d_color.p)
    same_floats(d_color.read(), want_color, what + ": composite")
    f_den, f_hist, f_color = Img(dev, shape=(h, w, 4)), Img(dev, hist), Img(dev, color)
    Dn.resolve_reflections(ctx, p, w, h, d_refl.p, d_depth.p, d_guide.p, f_hist.p, f_color.p, f_den.p)
    for got, three, name in ((f_den, d_den, "denoised"), (f_hist, d_hist, "history"), (f_color, d_color, "colour")):
        np.testing.assert_array_equal(words(got.read()), words(three.read()), err_msg=what + ": fused " + name)
    for img, src in ((d_refl, refl), (d_depth, depth), (d_guide, guide)):                 # only read
        np.testing.assert_array_equal(words(img.read()), words(np.ascontiguousarray(src, dtype=F)))
    return want_den, want_hist, want_color


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_sizes_kinds_and_radii(gpu, size):
    """1. Images around the tile's edge, one smaller than the halo, more than one workgroup; both normal kinds, r = 1 .. 4."""
    ctx, dev = gpu
    w, h = size
    for kind in KINDS:
        refl, depth, guide, hist, color = images(w, h, 31 * w + h + kind, kind)
        for radius in (1, 2, 3, 4):
            p = Dn.params(normal_kind=kind, has_history=radius != 3, kernel_radius=radius, inv_view=rotation() if radius & 1 else None)
            den, _, col = run_all(ctx, dev, p, refl, depth, guide, hist, color, f"{w}x{h} kind {kind} r {radius}")
            if w * h > 100:
                assert (den != 0).any() and (words(col) != words(color)).any()
        release(dev)


def edge_base(kind):
    refl, depth, guide, hist, color = images(17, 17, 900 + kind, kind)
    refl[..., 3] = np.maximum(refl[..., 3], F(0.05))
    depth = np.minimum(depth, F(0.9))
    return refl, depth, guide, hist, color


@pytest.mark.parametrize("kind", KINDS)
def test_edge_inputs(gpu, kind):
    """2. Hand-made on 17 x 17, one at a time and all of them against the restatement."""
    ctx, dev = gpu
    p = Dn.params(normal_kind=kind, has_history=True)
    below_one = np.nextafter(F(1), F(0))

    def centre_alpha_0(r, d, g):
        r[8, 8, 3] = 0

    def centre_alpha_minus_0(r, d, g):
        r[8, 8, 3] = -0.0

    def centre_depth_1(r, d, g):
        d[8, 8] = 1.0

    def centre_depth_below_1(r, d, g):
        d[8, 8] = below_one

    def neighbours_alpha_0(r, d, g):
        keep = r[8, 8, 3]
        r[4:13, 4:13, 3] = 0
        r[8, 8, 3] = keep

    def zero_normals(r, d, g):
        g[..., :3] = 0                                                                     # WORLD: dot = 0, every weight 0: the fallback

    def opposed_normals(r, d, g):
        g[8, 8, :3] = (0, 0, 1) if kind == Dn.NORMAL_WORLD else (0.5, 0.5, 0)
        g[8, 9, :3] = (0, 0, -1) if kind == Dn.NORMAL_WORLD else (0.0, 0.0, 0)             # octahedral (0, 0) decodes to -z

    def nan_colour_in_a_tap(r, d, g):
        r[7, 9, 1] = np.nan

    def corner(r, d, g):
        r[0, 0] = (0.9, 0.1, 0.4, 0.7)                                                      # every out-of-range tap of (0, 0) is (0, 0)

    edits = [centre_alpha_0, centre_alpha_minus_0, centre_depth_1, centre_depth_below_1, neighbours_alpha_0, zero_normals, opposed_normals,
             nan_colour_in_a_tap, corner]
    for edit in edits:
        refl, depth, guide, hist, color = edge_base(kind)
        edit(refl, depth, guide)
        den, nh, col = run_all(ctx, dev, p, refl, depth, guide, hist, color, edit.__name__)
        if edit in (centre_alpha_0, centre_alpha_minus_0, centre_depth_1):
            assert (den[8, 8] == 0).all()
        if edit is centre_depth_below_1:
            assert (den[8, 8] != 0).any()
        if edit is neighbours_alpha_0:
            assert np.allclose(den[8, 8], refl[8, 8], rtol=2.0 ** -22, atol=0)             # the centre tap alone: (c * w) / w, two roundings
        if edit is zero_normals and kind == Dn.NORMAL_WORLD:
            np.testing.assert_array_equal(words(den), words(refl))                         # weight_sum = 0 <= 0.001: the centre colour
        if edit is nan_colour_in_a_tap:
            # the tap's weight is a NaN, so weight_sum is one, `weight_sum > 0.001f` is false and every pixel the tap reaches falls back
            # to its own centre colour, as the shader's select does: the NaN itself appears only where it was put
            np.testing.assert_array_equal(words(den[5:10, 7:12]), words(refl[5:10, 7:12]))
            assert np.isnan(den[7, 9, 1]) and np.isnan(den).sum() == 1
            assert (words(den[4, 9]) != words(refl[4, 9])).any()                            # out of the tap's reach: filtered
        release(dev)


def test_temporal_branches(gpu):
    """3. The four branches with |cur.a - hist.a| at the threshold and one ulp to either side; in place against out of place; five
    frames in sequence."""
    ctx, dev = gpu
    w, h = 17, 5
    rng = np.random.default_rng(77)
    cur = rng.uniform(0.1, 1, (h, w, 4)).astype(F)
    hist = rng.uniform(0.1, 1, (h, w, 4)).astype(F)
    # a threshold whose neighbours are differences of float32 pairs: 0.1875 and 0.21875 share the ulp 2^-26, and x - 0.03125 is exact
    thr, low = F(0.1875), F(0.03125)
    pick = np.array([F(0.21875), np.nextafter(F(0.21875), F(0)), np.nextafter(F(0.21875), F(1))], F)
    assert list(pick - low) == [thr, np.nextafter(thr, F(0)), np.nextafter(thr, F(1))]
    cur[0, 0:3, 3], hist[0, 0:3, 3] = low, pick
    cur[0, 3:6, 3], hist[0, 3:6, 3] = pick, low
    cur[1, 0:4, 3] = (0, -0.0, -1, 0.3)
    hist[1, 4:8, 3] = (0, -0.0, -1, 0.3)
    cur[1, 8, 3], hist[1, 8, 3] = 0, 0                                                     # both: the decay wins
    cur[2, 0, 0], hist[2, 1, 2] = np.nan, np.inf
    for has in (True, False):
        p = Dn.params(has_history=has, depth_threshold=float(thr))
        want = Dn.temporal(p, cur, hist)
        d_cur, d_hist, d_out = Img(dev, cur), Img(dev, hist), Img(dev, shape=cur.shape)
        Dn.denoise_temporal(ctx, p, w, h, d_cur.p, d_hist.p, d_out.p)
        same_floats(d_out.read(), want, f"out of place, history {has}")
        np.testing.assert_array_equal(words(d_hist.read()), words(hist))
        Dn.denoise_temporal(ctx, p, w, h, d_cur.p, d_hist.p, d_hist.p)
        np.testing.assert_array_equal(words(d_hist.read()), words(d_out.read()), err_msg="in place")
        if has:
            a = F(p.blend_factor)
            kept = hist[0, 1] * (F(1) - a) + cur[0, 1] * a
            np.testing.assert_array_equal(words(want[0, 1]), words(kept))                  # just under the threshold: blended
            assert (words(want[0, 4]) != words(cur[0, 4])).any()
            for x in (0, 2, 3, 5):                                                           # at or over it: rejected, the current pixel
                np.testing.assert_array_equal(words(want[0, x]), words(hist[0, x] * F(0) + cur[0, x] * F(1)))
            np.testing.assert_array_equal(words(want[1, 0]), words(hist[1, 0] * F(0.9)))
            np.testing.assert_array_equal(words(want[1, 4]), words(cur[1, 4]))
            np.testing.assert_array_equal(words(want[1, 8]), words(hist[1, 8] * F(0.9)))
    # five frames
    p = Dn.params(has_history=False)
    d_hist, want = Img(dev, shape=cur.shape), None
    for f in range(5):
        frame = rng.uniform(0, 1, (h, w, 4)).astype(F)
        frame[..., 3] = np.where(rng.uniform(0, 1, (h, w)) < 0.3, 0, frame[..., 3])
        p.has_history = int(f > 0)
        want = Dn.temporal(p, frame, want)
        Dn.denoise_temporal(ctx, p, w, h, Img(dev, frame).p, d_hist.p, d_hist.p)
        same_floats(d_hist.read(), want, f"frame {f}")
    release(dev)


@pytest.mark.parametrize("kind", KINDS)
def test_composite_clamps(gpu, kind):
    """4. Untouched pixels keep every bit; alpha 0.001 and the float above it; roughness 0, at the threshold and beyond; NdotV at its
    clamp; a rotated inv_view and the identity."""
    ctx, dev = gpu
    w, h = 17, 9
    refl, depth, guide, _, color = images(w, h, 55 + kind, kind)
    refl[..., 3] = np.maximum(refl[..., 3], F(0.3))
    depth = np.minimum(depth, F(0.9))
    rough = 2 if kind == Dn.NORMAL_OCTAHEDRAL else 3
    refl[0, 0, 3], refl[0, 1, 3], refl[0, 2, 3] = F(0.001), np.nextafter(F(0.001), F(1)), 0
    depth[0, 3], depth[0, 4] = 1.0, np.nextafter(F(1), F(0))
    guide[1, 0, rough], guide[1, 1, rough], guide[1, 2, rough], guide[1, 3, rough] = 0, F(0.3), np.nextafter(F(0.3), F(1)), 0.9
    guide[2, 0:4, rough] = 0
    guide[0, 0:5, rough] = 0
    if kind == Dn.NORMAL_WORLD:
        guide[2, 0, :3], guide[2, 1, :3], guide[2, 2, :3] = (0, 0, -1), (0, 0, 1), (1, 0, 0)   # facing away: NdotV clamps to 0.001
    else:
        guide[2, 0, :2], guide[2, 1, :2] = (0, 0), (0.5, 0.5)
    color[3, 3] = (np.nan, -0.0, np.inf, 0.25)
    words(color)[4, 4, 3] = 0x7FC12345
    for inv_view in (None, rotation()):
        p = Dn.params(normal_kind=kind, inv_view=inv_view)
        want = Dn.composite(p, refl, depth, guide, color)
        d_color = Img(dev, color)
        Dn.composite_reflections(ctx, p, w, h, Img(dev, refl).p, Img(dev, depth).p, Img(dev, guide).p, d_color.p)
        got = d_color.read()
        same_floats(got, want, f"inv_view {'rotated' if inv_view is not None else 'identity'}")
        for x in (0, 2, 3):
            np.testing.assert_array_equal(words(got[0, x]), words(color[0, x]))            # untouched: every bit
        assert (words(got[0, 1]) != words(color[0, 1])).any() and (words(got[0, 4]) != words(color[0, 4])).any()
        np.testing.assert_array_equal(words(got[..., 3]), words(color[..., 3]))            # alpha kept, payload included
        for x in (1, 2, 3):                                                                  # smoothstep reaches 1: blend 0
            np.testing.assert_array_equal(got[1, x, :3], (color[1, x, :3] * F(1) + refl[1, x, :3] * F(0)))
        assert (got[1, 0, :3] != color[1, 0, :3]).any()
    release(dev)


def test_fused_over_three_frames(gpu):
    """5. mrt_resolve_reflections equals the three calls in sequence word for word on 33 x 17 over three frames, with and without
    d_denoised."""
    ctx, dev = gpu
    w, h = 33, 17
    for kind in KINDS:
        _, depth, guide, _, color = images(w, h, 3 + kind, kind)
        d_depth, d_guide = Img(dev, depth), Img(dev, guide)
        three = dict(hist=Img(dev, shape=(h, w, 4)), color=Img(dev, color), den=Img(dev, shape=(h, w, 4)))
        fused = dict(hist=Img(dev, shape=(h, w, 4)), color=Img(dev, color), den=Img(dev, shape=(h, w, 4)))
        bare = dict(hist=Img(dev, shape=(h, w, 4)), color=Img(dev, color))
        want_hist, want_color = None, color
        for f in range(3):
            refl = images(w, h, 40 + 7 * f + kind, kind)[0]
            p = Dn.params(normal_kind=kind, has_history=f > 0, inv_view=rotation(), kernel_radius=2 + (f & 1))
            d_refl = Img(dev, refl)
            Dn.denoise_spatial(ctx, p, w, h, d_refl.p, d_depth.p, d_guide.p, three["den"].p)
            Dn.denoise_temporal(ctx, p, w, h, three["den"].p, three["hist"].p, three["hist"].p)
            Dn.composite_reflections(ctx, p, w, h, three["hist"].p, d_depth.p, d_guide.p, three["color"].p)
            Dn.resolve_reflections(ctx, p, w, h, d_refl.p, d_depth.p, d_guide.p, fused["hist"].p, fused["color"].p, fused["den"].p)
            Dn.resolve_reflections(ctx, p, w, h, d_refl.p, d_depth.p, d_guide.p, bare["hist"].p, bare["color"].p)
            _, want_hist, want_color = Dn.resolve(p, refl, depth, guide, want_hist, want_color)
            for k in ("hist", "color", "den"):
                np.testing.assert_array_equal(words(fused[k].read()), words(three[k].read()), err_msg=f"frame {f} {k}")
                if k in bare:
                    np.testing.assert_array_equal(words(bare[k].read()), words(three[k].read()), err_msg=f"frame {f} {k}, no d_denoised")
            same_floats(three["hist"].read(), want_hist, f"frame {f} history")
            same_floats(three["color"].read(), want_color, f"frame {f} colour")
        assert (words(want_color) != words(color)).any()
        release(dev)


W, H = 64, 48
ROOM_ORIGIN, ROOM_FWD, ROOM_FOV = (0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0
FAR = F(1e30)


def reflected_frame(rays, hits, reflection_hits, shade, lights, env, inv_range, p, hist, mask=None):
    """One reflected frame of the W x H grid in numpy from the primary rays and their records: the rows, the lit frame (mask: the primary shadow mask
    [lights, n] or None), the reflection rays, reflection_hits(rrays) -> their records, their rows and lit frame, the guides, and
    Dn.resolve with the history `hist` (None on the first frame).  Returns a dict of every stage."""
    hit = hits["prim_id"] != -1
    rows = expected(rays, hits, shade)[0]
    lit = Lg.shade_linear(rows, hit, hit_point(rays, hits), rays["direction"], lights, mask, env)[0]
    rrays = R.reflection_rays(rays["direction"], hit_point(rays, hits), hits["normal"], hit, FAR)[0]
    rhits = reflection_hits(rrays)
    rhit = rhits["prim_id"] != -1
    rrows = expected(rrays, rhits, shade)[0]
    rlit = Lg.shade_linear(rrows, rhit, hit_point(rrays, rhits), rrays["direction"], lights, None, env)[0]
    depth, guide = Dn.guides(hits, rows, inv_range)
    _, new_hist, color = Dn.resolve(p, rlit.reshape(H, W, 4), depth.reshape(H, W), guide.reshape(H, W, 4), hist, lit.reshape(H, W, 4))
    return dict(hit=hit, rows=rows, lit=lit, rrays=rrays, rhits=rhits, rrows=rrows, rlit=rlit, depth=depth, guide=guide, hist=new_hist, color=color)


def test_guides_and_a_reflected_frame_end_to_end(built):
    """6, 7. synth.room() at 64 x 48: primary cast -> resolve -> light -> reflection cast -> resolve -> light -> mrt_reflection_guides
    -> mrt_resolve_reflections, all on the device, two frames, against the same chain in numpy on the device's records.  The primary cast
    sees layer 1 alone (the sphere and the boxes), so the room's walls are its misses; the reflection rays see everything."""
    sc = scene("room")
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        shade = shade_data("room")
        upload(ctx, shade)
        lights, env = light_list("room")[:4], environment()
        n = W * H
        cam = capi.camera_look(ROOM_ORIGIN, ROOM_FWD, W, H, ROOM_FOV)
        rays = po.grid_rays(ROOM_ORIGIN, ROOM_FWD, W, H, ROOM_FOV)
        d_hits, d_rows, d_lit = dev.alloc(n * 32), dev.alloc(n * 64), Img(dev, shape=(H, W, 4))
        d_rhits, d_rrays, d_rrows, d_rlit = dev.alloc(n * 32), dev.alloc(n * 32), dev.alloc(n * 64), Img(dev, shape=(H, W, 4))
        d_depth, d_guide, d_hist = Img(dev, shape=(H, W)), Img(dev, shape=(H, W, 4)), Img(dev, shape=(H, W, 4))
        inv_range = F(1.0 / 12.0)
        want_hist = None
        for frame in range(2):
            ctx.cast_grid(cam, W, H, hits=d_hits, query_mask=1, flags=capi.FLAG_HITS_ON_DEVICE)     # layer 1: the sphere and the boxes; the walls are misses
            ctx.resolve_grid_surfaces(cam, W, H, d_hits, d_rows)
            ctx.light_grid_surfaces(cam, W, H, d_hits, d_rows, lights, d_lit.p, None, env)
            ctx.cast_grid_reflections(cam, W, H, d_hits, d_rhits, FAR, d_out_rays=d_rrays)
            ctx.resolve_surfaces(d_rrays, d_rhits, n, d_rrows)
            ctx.light_surfaces(d_rrays, d_rhits, d_rrows, n, lights, d_rlit.p, None, env)
            Dn.reflection_guides(ctx, d_hits, d_rows, n, inv_range, d_depth.p, d_guide.p)
            p = Dn.params(normal_kind=Dn.NORMAL_WORLD, has_history=frame > 0, roughness_threshold=0.9, intensity=2.0)
            color, refl = d_lit.read().copy(), d_rlit.read().copy()
            Dn.resolve_reflections(ctx, p, W, H, d_rlit.p, d_depth.p, d_guide.p, d_hist.p, d_lit.p)
            # the same chain in numpy, on the device's records
            hits = dev.get(d_hits, n, T.HIT32)
            want = reflected_frame(rays, hits, lambda rrays: dev.get(d_rhits, n, T.HIT32), shade, lights, env, inv_range, p, want_hist)
            hit, lit, depth, guide = want["hit"], want["lit"], want["depth"], want["guide"]
            assert hit.any() and (~hit).any()                                              # misses included
            same(dev.get(d_rows, n, T.SURFACE64), want["rows"])
            np.testing.assert_array_equal(words(color.reshape(-1, 4)), words(lit))
            same(dev.get(d_rrays, n, T.RAY32), want["rrays"])
            np.testing.assert_array_equal(words(refl.reshape(-1, 4)), words(want["rlit"]))
            np.testing.assert_array_equal(words(d_depth.read().reshape(-1)), words(depth))
            np.testing.assert_array_equal(words(d_guide.read().reshape(-1, 4)), words(guide))
            assert (depth[~hit] == 1).all() and (depth[hit] < 1).any() and (guide[~hit] == 0).all()
            want_hist, want_color = want["hist"], want["color"]
            same_floats(d_hist.read(), want_hist, f"frame {frame} history")
            same_floats(d_lit.read(), want_color, f"frame {frame} colour")
            assert (words(want_color) != words(lit.reshape(H, W, 4))).any()                 # reflections were blended in
    finally:
        dev.free()
        ctx.close()


def test_async_refusals_pending_and_primary_grids(built):
    """8. MRT_FLAG_ASYNC then mrt_synchronize; every kind of refusal with a context, nothing written; W or H 0; a pending dispatch; a
    primary grid cast before and after is unchanged."""
    L = Dn.lib()
    L.mrt_last_error.restype = C.c_char_p
    sc = scene("soup")
    gw, gh = 100, 77
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        o, f, fov = sc.cam
        cam = capi.camera_look(o, f, gw, gh, fov)
        rays = po.grid_rays(o, f, gw, gh, fov)
        sc.upload(ctx)
        first = ctx.cast_grid(cam, gw, gh)
        kernel = (ctx.stats()["last_kernel"], ctx.last_kernel_variant())
        w, h = 33, 17
        refl, depth, guide, hist, color = images(w, h, 1, 0)
        d_refl, d_depth, d_guide = Img(dev, refl), Img(dev, depth), Img(dev, guide)
        out, d_hist, d_color = Img(dev, shape=(h, w, 4)), Img(dev, shape=(h, w, 4)), Img(dev, shape=(h, w, 4))
        p = Dn.params()

        def spatial(pp=p, ww=w, hh=h, r=d_refl.p, d=d_depth.p, g=d_guide.p, o_=out.p, flags=0):
            return L.mrt_denoise_spatial(ctx.h, C.byref(pp) if pp is not None else None, ww, hh, r, d, g, o_, flags)

        def fused(pp=p, ww=w, hh=h, r=d_refl.p, d=d_depth.p, g=d_guide.p, hi=d_hist.p, c=d_color.p, den=None, flags=0):
            return L.mrt_resolve_reflections(ctx.h, C.byref(pp), ww, hh, r, d, g, hi, c, den, flags)

        def refused(rc, word):
            return rc == capi.ERR_INVALID and word in L.mrt_last_error(ctx.h)

        assert refused(spatial(pp=None), b"null params") and refused(spatial(r=None), b"null d_reflection") and refused(spatial(o_=None), b"null d_out")
        assert refused(spatial(pp=Dn.params(struct_size=108)), b"struct_size")
        for fl in (capi.FLAG_BOOL_OUT, capi.FLAG_COHERENT, capi.FLAG_HOST_LAYOUT, 1 << 20):
            assert refused(spatial(flags=fl), b"flag")
        assert refused(spatial(pp=Dn.params(normal_kind=2)), b"normal_kind")
        assert refused(spatial(pp=Dn.params(color_sigma=float("nan"))), b"non-finite") and refused(spatial(pp=Dn.params(f0=float("inf"))), b"non-finite")
        assert refused(spatial(ww=0xFFFFFFFF, hh=0xFFFFFFFF), b"overflows")
        assert refused(spatial(o_=d_refl.p), b"d_out is d_reflection")
        assert refused(fused(hi=d_refl.p), b"across pixels") and refused(fused(c=d_guide.p), b"across pixels") and refused(fused(den=d_depth.p), b"across pixels")
        # the order: wrong in everything
        worst = Dn.params(struct_size=1, normal_kind=9, depth_sigma=float("nan"))
        assert refused(spatial(pp=worst, g=None, flags=1 << 20, ww=0xFFFFFFFF, hh=0xFFFFFFFF, o_=d_refl.p), b"null d_normal_roughness")
        assert refused(spatial(pp=worst, flags=1 << 20, ww=0xFFFFFFFF, hh=0xFFFFFFFF, o_=d_refl.p), b"struct_size")
        worst.struct_size = 112
        assert refused(spatial(pp=worst, flags=1 << 20, ww=0xFFFFFFFF, hh=0xFFFFFFFF, o_=d_refl.p), b"flag")
        assert refused(spatial(pp=worst, ww=0xFFFFFFFF, hh=0xFFFFFFFF, o_=d_refl.p), b"normal_kind")
        worst.normal_kind = 1
        assert refused(spatial(pp=worst, ww=0xFFFFFFFF, hh=0xFFFFFFFF, o_=d_refl.p), b"non-finite")
        worst.depth_sigma = 1.0
        assert refused(spatial(pp=worst, ww=0xFFFFFFFF, hh=0xFFFFFFFF, o_=d_refl.p), b"overflows")
        assert refused(spatial(pp=worst, o_=d_refl.p), b"d_out is d_reflection")
        assert refused(L.mrt_reflection_guides(ctx.h, None, d_refl.p, 4, 1.0, d_depth.p, d_guide.p, 0), b"null d_hits")
        assert refused(L.mrt_reflection_guides(ctx.h, d_refl.p, d_refl.p, 4, float("inf"), d_depth.p, out.p, 0), b"non-finite")
        assert spatial(ww=0) == capi.MRT_OK and spatial(hh=0) == capi.MRT_OK and fused(ww=0, hh=0) == capi.MRT_OK
        assert L.mrt_reflection_guides(ctx.h, d_refl.p, d_refl.p, 0, 1.0, d_depth.p, out.p, 0) == capi.MRT_OK
        assert out.untouched() and d_hist.untouched() and d_color.untouched()
        # a pending dispatch
        ctx.submit(rays)
        assert spatial() == capi.ERR_PENDING and fused() == capi.ERR_PENDING
        assert L.mrt_denoise_temporal(ctx.h, C.byref(p), w, h, d_refl.p, d_hist.p, out.p, 0) == capi.ERR_PENDING
        assert L.mrt_composite_reflections(ctx.h, C.byref(p), w, h, d_refl.p, d_depth.p, d_guide.p, d_color.p, 0) == capi.ERR_PENDING
        assert L.mrt_reflection_guides(ctx.h, d_refl.p, d_refl.p, 4, 1.0, d_depth.p, out.p, 0) == capi.ERR_PENDING
        assert out.untouched() and d_hist.untouched() and d_color.untouched()
        ctx.collect()
        stats = ctx.stats()
        # ASYNC: the three calls queued, then one wait
        a_hist, a_color = Img(dev, hist), Img(dev, color)
        p2 = Dn.params(has_history=True, inv_view=rotation())
        Dn.denoise_spatial(ctx, p2, w, h, d_refl.p, d_depth.p, d_guide.p, out.p, flags=capi.FLAG_ASYNC)
        Dn.denoise_temporal(ctx, p2, w, h, out.p, a_hist.p, a_hist.p, flags=capi.FLAG_ASYNC)
        Dn.composite_reflections(ctx, p2, w, h, a_hist.p, d_depth.p, d_guide.p, a_color.p, flags=capi.FLAG_ASYNC)
        ctx.synchronize()
        b_hist, b_color = Img(dev, hist), Img(dev, color)
        Dn.resolve_reflections(ctx, p2, w, h, d_refl.p, d_depth.p, d_guide.p, b_hist.p, b_color.p, flags=capi.FLAG_ASYNC)
        ctx.synchronize()
        want = Dn.resolve(p2, refl, depth, guide, hist, color)
        for got, wnt in ((out, want[0]), (a_hist, want[1]), (a_color, want[2]), (b_hist, want[1]), (b_color, want[2])):
            same_floats(got.read(), wnt, "async")
        # the scene, the statistics and the next primary grid are as they were
        assert ctx.stats() == stats
        again = ctx.cast_grid(cam, gw, gh)
        same(again, first)
        assert (ctx.stats()["last_kernel"], ctx.last_kernel_variant()) == kernel
    finally:
        dev.free()
        ctx.close()
