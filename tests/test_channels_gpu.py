"""mrt_shade_channels / mrt_shade_grid_channels, mrt_finish_color and mrt_image_to_rgba8: the renderer's ten channels besides COLOR, the
last pass of a lit frame and the 8-bit image on the device, held to the numpy float32 restatement (messyerraytracer_amd/channels.py;
pinned to the reference by test_channels_cpu.py) byte for byte -- float planes as uint32 words, byte planes as bytes.  The scenes, grids,
shade data and textures of test_texture_gpu.py; guard words behind every plane."""
import ctypes as C
import os

import numpy as np
import pytest

from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import channels as Ch
from messyerraytracer_amd import surface as S
from messyerraytracer_amd import texture as X
from oracle import pyoracle as po
from test_hemisphere_gpu import DEV, Dev, Run, same, scene
from test_lighting_gpu import Lit
from test_surface_gpu import GRIDS, GRID_IDS, ID_PERIOD, KINDS, N_MATERIALS, shade_data, without
from test_texture_gpu import texture_set, textured_shade

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
PATTERN = 0xA5A5A5A5
INV_POS = F(1) / F(0.75)
N_FRAME = 8 * 257                 # the records of the shared frame that are restated: eight rows of its grid
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "channels_reference.npz")


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def inv_depth(hits):
    """1 / (median hit t): about half of the hits lie beyond the range"""
    return F(1) / F(np.median(hits["t"][hits["prim_id"] != -1]))


def expected(rays, hits, shade, tex, inv_d, inv_p=INV_POS, channels=Ch.ALL):
    """the planes of mrt_ray32 rays and mrt_hit32 records"""
    return Ch.shade_channels(rays["direction"], Ch.hit_position(rays["origin"], rays["direction"], hits["t"]), hits["normal"],
                             hits["prim_id"] != -1, hits["t"], hits["prim_id"].view(np.uint32), hits["bary_u"], hits["bary_v"],
                             inv_d, inv_p, shade, tex, channels)


class Planes:
    """float and / or byte planes of some channels on the device, a guard behind each"""

    def __init__(self, dev, n, channels=Ch.ALL, floats=True, bytes8=True):
        self.dev, self.n = dev, n
        self.rgba = {c: dev.put(np.full(n * 4 + GUARD, PATTERN, np.uint32)) for c in channels} if floats else {}
        self.rgba8 = {c: dev.put(np.full(n + GUARD, PATTERN, np.uint32)) for c in channels} if bytes8 else {}

    def check(self, want):
        n = self.n
        for c, p in self.rgba.items():
            got = self.dev.get(p, n * 4 + GUARD, np.uint32)
            assert (got[n * 4:] == PATTERN).all(), c
            np.testing.assert_array_equal(got[:n * 4].reshape(-1, 4), words(want[c]), err_msg=f"channel {c}")
        for c, p in self.rgba8.items():
            got = self.dev.get(p, n + GUARD, np.uint32)
            assert (got[n:] == PATTERN).all(), c
            np.testing.assert_array_equal(got[:n].view(np.uint8).reshape(-1, 4), Ch.to_rgba8(want[c]), err_msg=f"channel {c} bytes")

    def untouched(self):
        return all((self.dev.get(p, self.n * k + GUARD, np.uint32) == PATTERN).all()
                   for planes, k in ((self.rgba, 4), (self.rgba8, 1)) for p in planes.values())


def grid_call(run, planes, inv_d, inv_p=INV_POS, flags=0):
    run.ctx.shade_grid_channels(run.cam, run.w, run.h, run.d_hits, inv_d, inv_p, planes.rgba, planes.rgba8, y0=run.y0, y1=run.y1, flags=flags)
    return planes


def assert_cases_occur(kind, rays, hits, shade, tex, inv_d):
    hit = hits["prim_id"] != -1
    prim = hits["prim_id"].view(np.uint32)
    u, v = hits["bary_u"][hit], hits["bary_v"][hit]
    w = (F(1) - u) - v
    s = (np.minimum(np.minimum(w, u), v) - F(0.01)) / (F(0.03) - F(0.01))
    assert (s < 0).any() and ((s > 0) & (s < 1)).any() and (s > 1).any(), "wireframe: below, inside and above the ramp"
    x = F(1) - hits["t"][hit] * inv_d
    assert (x < 0).any() and ((x > 0) & (x < 1)).any(), "depth: beyond the range and inside it"
    x = F(1) - hits["t"][hit] * -inv_d
    assert (x > 1).any(), "depth: the clamp at 1 (the negated range)"
    assert (Ch.hit_position(rays["origin"], rays["direction"], hits["t"])[hit] < 0).any(), "a negative position coordinate"
    rows, _, ns = S.resolve(rays["direction"], hits["normal"], hit, prim, hits["bary_u"], hits["bary_v"], shade)
    trows, _, n = X.resolve_textured(rays["direction"], hits["normal"], hit, prim, hits["bary_u"], hits["bary_v"], shade, tex)
    in_range = hit & (prim < shade.n_tris)
    assert (rows["uv"][in_range] < 0).any(), "negative UVs"
    d = rays["direction"]
    q = (ns[:, 0] * -d[:, 0] + ns[:, 1] * -d[:, 1]) + ns[:, 2] * -d[:, 2]
    assert (q[hit] < 0).any() and ((q[hit] > 0) & (q[hit] < 1)).any(), "a fresnel clamp at 0"
    assert (words(n[hit]) != words(ns[hit])).any(), "a perturbed normal"
    assert (words(trows["albedo"][hit]) != words(rows["albedo"][hit])).any(), "a sampled albedo"
    assert (hit & ~in_range).any(), "a prim id out of range"
    assert (in_range & (prim % ID_PERIOD >= N_MATERIALS)).any(), "a material id out of range"
    if kind == "soup":
        assert (~hit).any(), "misses"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_every_form_matches_the_restatement(built, kind, grid):
    """1. All ten channels, float and byte planes: grid form, array form and host-layout array form; the depth channel also over the
    negated range (the clamp at 1, which no positive t reaches)."""
    run = Run(kind, *grid)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade, tex = textured_shade(kind), texture_set(kind)
        inv_d = inv_depth(run.hits)
        assert_cases_occur(kind, run.rays, run.hits, shade, tex, inv_d)
        ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
        ctx.upload_textures(tex.textures, tex.bindings, tex.tangents12)
        want = expected(run.rays, run.hits, shade, tex, inv_d)
        grid_call(run, Planes(dev, n), inv_d).check(want)
        neg = expected(run.rays, run.hits, shade, tex, -inv_d, channels=(Ch.DEPTH,))
        assert (neg[Ch.DEPTH][:, 0] == 1).any()
        grid_call(run, Planes(dev, n, (Ch.DEPTH,)), -inv_d).check(neg)
        # the array form on what mrt_cast read and wrote
        d_rays, d_h32 = dev.put(run.rays), dev.alloc(n * 32)
        ctx.cast(d_rays, d_h32, count=n, flags=DEV)
        same(dev.get(d_h32, n, T.HIT32), run.hits)
        o = Planes(dev, n)
        ctx.shade_channels(d_rays, d_h32, n, inv_d, INV_POS, o.rgba, o.rgba8)
        o.check(want)
        # the reference's host layout: the position is the record's own
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        want44 = Ch.shade_channels(hrays["direction"], h44["position"], h44["normal"], h44["prim_id"] != T.NO_HIT, h44["t"], h44["prim_id"],
                                   h44["u"], h44["v"], inv_d, INV_POS, shade, tex)
        o = Planes(dev, n)
        ctx.shade_channels(d_hr, d_h44, n, inv_d, INV_POS, o.rgba, o.rgba8, flags=capi.FLAG_HOST_LAYOUT)
        o.check(want44)
    finally:
        run.close()


class Frame:
    """One 257 x 256 soup grid with shade data and textures resident, and its planes restated once"""
    made = None

    def __init__(self):
        self.run = Run("soup", 257, 256)
        self.shade, self.tex = textured_shade("soup"), texture_set("soup")
        ctx = self.run.ctx
        ctx.upload_shade_data(self.shade.n_tris, self.shade.materials, self.shade.material_ids, self.shade.normals9, self.shade.uvs6)
        ctx.upload_textures(self.tex.textures, self.tex.bindings, self.tex.tangents12)
        self.inv_d = inv_depth(self.run.hits)
        self.d_rays = self.run.dev.put(self.run.rays)
        first = slice(0, N_FRAME)
        self.want = expected(self.run.rays[first], self.run.hits[first], self.shade, self.tex, self.inv_d)


@pytest.fixture(scope="module")
def frame(built):
    f = Frame()
    yield f
    f.run.close()


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_array_counts_at_the_workgroup_edge(frame, count):
    """2. The array form on the first `count` records: the planes end where the count ends."""
    run = frame.run
    o = Planes(run.dev, count)
    run.ctx.shade_channels(frame.d_rays, run.d_hits, count, frame.inv_d, INV_POS, o.rgba, o.rgba8)
    o.check({c: a[:count] for c, a in frame.want.items()})


@pytest.mark.parametrize("channel", Ch.ALL)
def test_each_channel_alone(frame, channel):
    """3. One channel, floats only and bytes only, both forms: its plane is right, every other plane keeps its pattern."""
    run, n = frame.run, N_FRAME
    for floats in (True, False):
        for array in (True, False):
            one, others = Planes(run.dev, n, (channel,), floats, not floats), Planes(run.dev, n, [c for c in Ch.ALL if c != channel])
            if array:
                run.ctx.shade_channels(frame.d_rays, run.d_hits, n, frame.inv_d, INV_POS, one.rgba, one.rgba8)
            else:
                run.ctx.shade_grid_channels(run.cam, run.w, run.h, run.d_hits, frame.inv_d, INV_POS, one.rgba, one.rgba8, y0=0, y1=8)
            one.check(frame.want)
            assert others.untouched()


@pytest.mark.parametrize("kind", ["soup", "room_tl"])
def test_absent_arrays_nothing_resident_and_textures_cleared(built, kind):
    """4. Nothing resident; each optional array absent in turn under the texture set; the textures cleared: all against the restatement."""
    run = Run(kind, 100, 77)
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        shade, tex = textured_shade(kind), texture_set(kind)
        inv_d = inv_depth(run.hits)
        grid_call(run, Planes(dev, n), inv_d).check(expected(run.rays, run.hits, None, None, inv_d))
        ctx.upload_textures(tex.textures, tex.bindings, tex.tangents12)
        grid_call(run, Planes(dev, n), inv_d).check(expected(run.rays, run.hits, None, tex, inv_d))
        for absent in ("ids", "normals", "uvs", "materials"):
            s = without(shade, absent)
            ctx.upload_shade_data(s.n_tris, s.materials, s.material_ids, s.normals9, s.uvs6)
            grid_call(run, Planes(dev, n), inv_d).check(expected(run.rays, run.hits, s, tex, inv_d))
        ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
        no_tangents = X.TextureSet(tex.textures, tex.bindings, None)
        ctx.upload_textures(no_tangents.textures, no_tangents.bindings, None)
        grid_call(run, Planes(dev, n), inv_d).check(expected(run.rays, run.hits, shade, no_tangents, inv_d))
        ctx.clear_textures()
        plain = expected(run.rays, run.hits, shade, None, inv_d)
        assert (words(plain[Ch.ALBEDO]) != words(expected(run.rays, run.hits, shade, tex, inv_d, channels=(Ch.ALBEDO,))[Ch.ALBEDO])).any()
        grid_call(run, Planes(dev, n), inv_d).check(plain)
        ctx.clear_shade_data()
        grid_call(run, Planes(dev, n), inv_d).check(expected(run.rays, run.hits, None, None, inv_d))
    finally:
        run.close()


def test_a_band_shades_what_the_whole_frame_shades(built):
    """5."""
    whole, band = Run("room", 128, 96), Run("room", 128, 96, 20, 70)
    try:
        shade, tex = textured_shade("room"), texture_set("room")
        inv_d = inv_depth(whole.hits)
        outs = []
        for run in (whole, band):
            run.ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
            run.ctx.upload_textures(tex.textures, tex.bindings, tex.tangents12)
            o = grid_call(run, Planes(run.dev, run.n), inv_d)
            outs.append(({c: run.dev.get(p, run.n * 4, np.uint32).reshape(-1, 4) for c, p in o.rgba.items()},
                         {c: run.dev.get(p, run.n, np.uint32) for c, p in o.rgba8.items()}))
        rows = slice(20 * 128, 70 * 128)
        for c in Ch.ALL:
            same(outs[0][0][c][rows], outs[1][0][c])
            same(outs[0][1][c][rows], outs[1][1][c])
    finally:
        whole.close()
        band.close()


def test_async_then_synchronize(frame):
    """6. MRT_FLAG_ASYNC followed by mrt_synchronize gives the same bytes, both forms and both image calls."""
    run, n = frame.run, N_FRAME
    a, b = Planes(run.dev, n), Planes(run.dev, n)
    run.ctx.shade_grid_channels(run.cam, run.w, run.h, run.d_hits, frame.inv_d, INV_POS, a.rgba, a.rgba8, y0=0, y1=8, flags=capi.FLAG_ASYNC)
    run.ctx.shade_channels(frame.d_rays, run.d_hits, n, frame.inv_d, INV_POS, b.rgba, b.rgba8, flags=capi.FLAG_ASYNC)
    d8, d_fin, d_fin8 = run.dev.alloc(n * 4), run.dev.alloc(n * 16), run.dev.alloc(n * 4)
    run.ctx.image_to_rgba8(b.rgba[Ch.NORMAL], n, d8, flags=capi.FLAG_ASYNC)
    run.ctx.finish_color(b.rgba[Ch.FRESNEL], n, d_fin, d_fin8, tonemap_mode=3, flags=capi.FLAG_ASYNC)
    run.ctx.synchronize()
    a.check(frame.want)
    b.check(frame.want)
    same(run.dev.get(d8, n * 4, np.uint8).reshape(-1, 4), Ch.to_rgba8(frame.want[Ch.NORMAL]))
    fin = Ch.finish_color(frame.want[Ch.FRESNEL], 3)
    same(run.dev.get(d_fin, n * 4, F).reshape(-1, 4), fin)
    same(run.dev.get(d_fin8, n * 4, np.uint8).reshape(-1, 4), Ch.to_rgba8(fin))


def test_full_chain_to_a_finished_frame(built):
    """7. resolve -> shadows -> light with an environment -> mrt_finish_color, all five tone mappers: channels.finish_color of the lit
    frame; misses keep the sky's bits; in place; bytes alone."""
    lit = Lit("soup", 100, 77)
    run = lit.run
    dev, n = run.dev, run.n
    try:
        d_lit = dev.alloc(n * 16)
        lit.grid(d_lit)
        frame = dev.get(d_lit, n * 4, F).reshape(-1, 4)
        np.testing.assert_array_equal(words(frame), words(lit.want()))
        miss = ~lit.hit
        assert miss.any() and (frame[miss, 3] == 0).all() and (frame[lit.hit, 3] == 1).all()
        for mode in range(5):
            want = Ch.finish_color(frame, mode)
            np.testing.assert_array_equal(words(want[miss, :3]), words(frame[miss, :3]))
            d_out = dev.put(np.full(n * 4 + GUARD, PATTERN, np.uint32))
            d_out8 = dev.put(np.full(n + GUARD, PATTERN, np.uint32))
            run.ctx.finish_color(d_lit, n, d_out, d_out8, tonemap_mode=mode)
            got, got8 = dev.get(d_out, n * 4 + GUARD, np.uint32), dev.get(d_out8, n + GUARD, np.uint32)
            assert (got[n * 4:] == PATTERN).all() and (got8[n:] == PATTERN).all()
            np.testing.assert_array_equal(got[:n * 4].reshape(-1, 4), words(want))
            np.testing.assert_array_equal(got8[:n].view(np.uint8).reshape(-1, 4), Ch.to_rgba8(want))
            same(dev.get(d_lit, n * 4, F).reshape(-1, 4), frame)                           # the lit frame is only read
            d_only8 = dev.alloc(n * 4)                                                      # bytes alone
            run.ctx.finish_color(d_lit, n, None, d_only8, tonemap_mode=mode)
            same(dev.get(d_only8, n * 4, np.uint8).reshape(-1, 4), Ch.to_rgba8(want))
            d_place = dev.put(frame)                                                        # in place
            run.ctx.finish_color(d_place, n, d_place, tonemap_mode=mode)
            np.testing.assert_array_equal(words(dev.get(d_place, n * 4, F).reshape(-1, 4)), words(want))
    finally:
        lit.close()


def test_image_to_rgba8_on_the_fixtures_values(built):
    """8. The recorded to_image inputs (NaNs, infinities and -0.0f among them) give the recorded bytes."""
    g = np.load(GOLDEN)
    b_in, b_out = g["b_in"], g["b_out"]
    assert np.isnan(b_in).any() and np.isinf(b_in).any() and (words(b_in) == 0x80000000).any() and b_in.shape[0] % 4 == 0
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        n = b_in.shape[0] // 4
        d_in, d_out = dev.put(b_in), dev.put(np.full(n + GUARD, PATTERN, np.uint32))
        ctx.image_to_rgba8(d_in, n, d_out)
        got = dev.get(d_out, n + GUARD, np.uint32)
        assert (got[n:] == PATTERN).all()
        np.testing.assert_array_equal(got[:n].view(np.uint8), b_out)
    finally:
        dev.free()
        ctx.close()


def test_refusals_count_zero_and_pending(built):
    """9. Every refusal and their order, with and without a scene, before anything is written; count == 0 and an empty band are OK and
    write nothing; no scene is needed; a pending dispatch."""
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
        planes = Planes(dev, n)
        d_img, d_img8 = dev.put(np.full(n * 4 + GUARD, PATTERN, np.uint32)), dev.put(np.full(n + GUARD, PATTERN, np.uint32))
        R, Hp = C.c_void_p(d_rays), C.c_void_p(d_hits)
        good = capi.channel_out(0.25, 1.0, planes.rgba, planes.rgba8)
        nan, inf = float("nan"), float("inf")

        def desc(inv_d=0.25, inv_p=1.0, size=None, color=None, empty=False):
            d = capi.channel_out(inv_d, inv_p, None if empty else planes.rgba, None if empty else planes.rgba8)
            if size is not None:
                d.struct_size = size
            if color == "f":
                d.d_rgba[0] = d_img
            if color == "b":
                d.d_rgba8[0] = d_img8
            return d

        def arr(rays=R, hits=Hp, count=n, out=good, flags=0):
            return L.mrt_shade_channels(ctx.h, rays, hits, count, None if out is None else C.byref(out), flags)

        def grid(hits=Hp, out=good, flags=0, camera=cam, y0=0, y1=h):
            return L.mrt_shade_grid_channels(ctx.h, None if camera is None else C.byref(camera), w, h, y0, y1, hits,
                                             None if out is None else C.byref(out), flags)

        def untouched():
            return planes.untouched() and (dev.get(d_img, n * 4 + GUARD, np.uint32) == PATTERN).all() and (dev.get(d_img8, n + GUARD, np.uint32) == PATTERN).all()

        def bad_calls():
            common = [dict(hits=None), dict(out=None), dict(out=desc(size=184)), dict(out=desc(size=0)), dict(out=desc(color="f")),
                      dict(out=desc(color="b")), dict(out=desc(empty=True))]
            common += [dict(out=desc(inv_d=x)) for x in (nan, inf, -inf)] + [dict(out=desc(inv_p=x)) for x in (nan, inf, -inf)]
            for kw in common + [dict(rays=None)]:
                assert arr(**kw) == capi.ERR_INVALID, kw
            for kw in common + [dict(camera=None), dict(y0=10, y1=5), dict(y1=h + 1), dict(flags=capi.FLAG_HOST_LAYOUT)]:
                assert grid(**kw) == capi.ERR_INVALID, kw
            for fl in (capi.FLAG_BOOL_OUT, capi.FLAG_TOKEN_OUT, capi.FLAG_COHERENT, capi.FLAG_FORCE_SORT, capi.FLAG_RAYS_ON_DEVICE, 1 << 20):
                assert arr(flags=fl) == capi.ERR_INVALID and grid(flags=fl) == capi.ERR_INVALID, fl
                assert L.mrt_finish_color(ctx.h, d_rays, n, 0, d_img, d_img8, fl) == capi.ERR_INVALID
                assert L.mrt_image_to_rgba8(ctx.h, d_rays, n, d_img8, fl) == capi.ERR_INVALID
            assert L.mrt_finish_color(ctx.h, None, n, 0, d_img, d_img8, 0) == capi.ERR_INVALID
            assert L.mrt_finish_color(ctx.h, d_rays, n, 5, d_img, d_img8, 0) == capi.ERR_INVALID
            assert L.mrt_finish_color(ctx.h, d_rays, n, 0, None, None, 0) == capi.ERR_INVALID
            assert L.mrt_image_to_rgba8(ctx.h, None, n, d_img8, 0) == capi.ERR_INVALID
            assert L.mrt_image_to_rgba8(ctx.h, d_rays, n, None, 0) == capi.ERR_INVALID
            # the order, by the message of the first check that fails: struct_size before the flag before COLOR before the selection
            # before the ranges before the band
            everything = desc(inv_d=nan, size=8, color="f")
            assert grid(out=everything, flags=1 << 20, y0=10, y1=5) == capi.ERR_INVALID and b"struct_size" in L.mrt_last_error(ctx.h)
            everything.struct_size = C.sizeof(capi.ChannelOut)
            assert grid(out=everything, flags=1 << 20, y0=10, y1=5) == capi.ERR_INVALID and b"flag" in L.mrt_last_error(ctx.h)
            assert grid(out=everything, y0=10, y1=5) == capi.ERR_INVALID and b"COLOR" in L.mrt_last_error(ctx.h)
            assert grid(out=desc(inv_d=nan, empty=True), y0=10, y1=5) == capi.ERR_INVALID and b"no channel" in L.mrt_last_error(ctx.h)
            assert grid(out=desc(inv_d=nan), y0=10, y1=5) == capi.ERR_INVALID and b"finite" in L.mrt_last_error(ctx.h)
            assert grid(y0=10, y1=5) == capi.ERR_INVALID and b"grid" in L.mrt_last_error(ctx.h)
            assert L.mrt_finish_color(ctx.h, d_rays, n, 9, None, None, 1 << 20) == capi.ERR_INVALID and b"flag" in L.mrt_last_error(ctx.h)
            assert L.mrt_finish_color(ctx.h, d_rays, n, 9, None, None, 0) == capi.ERR_INVALID and b"tonemap" in L.mrt_last_error(ctx.h)

        L.mrt_last_error.restype = C.c_char_p
        bad_calls()                                   # no scene, nothing resident
        assert arr(count=0) == capi.MRT_OK and grid(y0=10, y1=10) == capi.MRT_OK
        assert L.mrt_finish_color(ctx.h, d_rays, 0, 0, d_img, d_img8, 0) == capi.MRT_OK and L.mrt_image_to_rgba8(ctx.h, d_rays, 0, d_img8, 0) == capi.MRT_OK
        assert untouched()
        # no scene is required: every hit against an empty SceneShadeData
        want = expected(rays, hits, None, None, F(0.25), F(1.0))
        assert grid() == capi.MRT_OK
        planes.check(want)
        sc.upload(ctx)
        planes = Planes(dev, n)
        good = capi.channel_out(0.25, 1.0, planes.rgba, planes.rgba8)
        bad_calls()
        assert untouched()
        # a pending dispatch
        ctx.submit(rays)
        assert arr(out=good) == capi.ERR_PENDING and grid(out=good) == capi.ERR_PENDING
        assert L.mrt_finish_color(ctx.h, d_rays, n, 0, d_img, d_img8, 0) == capi.ERR_PENDING
        assert L.mrt_image_to_rgba8(ctx.h, d_rays, n, d_img8, 0) == capi.ERR_PENDING
        assert untouched()
        ctx.collect()
        assert arr(out=good) == capi.MRT_OK
        planes.check(want)
    finally:
        dev.free()
        ctx.close()


def test_primary_grid_unaffected_by_channel_passes(built):
    """10. A renderer's frames: the primary grid with and without channel passes between frames -- the same kernel sequence, the same
    records."""
    sc = scene("room")
    w, h = 640, 480
    shade, tex = textured_shade("room"), texture_set("room")
    runs = []
    for shading in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
            ctx.upload_textures(tex.textures, tex.bindings, tex.tangents12)
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits = dev.alloc(w * h * 32)
            rgba = {c: dev.alloc(w * h * 16) for c in (Ch.NORMAL, Ch.DEPTH)}
            rgba8 = {c: dev.alloc(w * h * 4) for c in Ch.ALL}
            for f in range(8):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, w * h, T.HIT32).view(np.uint32))
                if shading:
                    fl = capi.FLAG_ASYNC if f & 1 else 0
                    ctx.shade_grid_channels(cam, w, h, d_hits, 0.125, INV_POS, rgba, rgba8, flags=fl)
                    ctx.finish_color(rgba[Ch.NORMAL], w * h, rgba[Ch.NORMAL], rgba8[Ch.NORMAL], tonemap_mode=3, flags=fl)
                    ctx.image_to_rgba8(rgba[Ch.DEPTH], w * h, rgba8[Ch.DEPTH], flags=fl)
            runs.append((kernels, records))
        finally:
            dev.free()
            ctx.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)


def test_two_to_the_sixteen_records(built):
    """11. 256 x 256 = 2^16 records."""
    run = Run("room_tl", 256, 256)
    try:
        shade, tex = textured_shade("room_tl"), texture_set("room_tl")
        inv_d = inv_depth(run.hits)
        assert_cases_occur("room_tl", run.rays, run.hits, shade, tex, inv_d)
        run.ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
        run.ctx.upload_textures(tex.textures, tex.bindings, tex.tangents12)
        grid_call(run, Planes(run.dev, run.n), inv_d).check(expected(run.rays, run.hits, shade, tex, inv_d))
    finally:
        run.close()
