"""Emissive triangles as light sources on the device: the emitter table against emitters.build_table word for word, from host and from
device arrays, over triangle counts around every block bound; more than MRT_MAX_EMITTERS emitters refused with the old table still
answering; mrt_cast_emitter_shadows / mrt_cast_grid_emitter_shadows held to emitters.emitter_samples (the words) and to the oracle's
any-hit answer for its rays, by the walk and by brute force (the mask bytes), on flat and two-level synth.room() and a soup, the grid
and a band of it, the array forms in both layouts, 1, 63, 65 and 4096 records on the plain kernels and 65 536 on the persistent ones;
mrt_light_emitter_surfaces and mrt_path_step_emitters held to the restatement as uint32 words, on resolved rows and on hand-made
records at the three refusals' thresholds; the emitter step against mrt_path_step; one whole frame of the queue INTEGRATION gives,
every state word against the numpy loop; refusals in the header's order; ASYNC on a caller's stream."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import bounce as B
from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import emitters as E
from messyerraytracer_amd import path as P
from messyerraytracer_amd import surface as S
from oracle import pyoracle as po
from test_caller_stream_gpu import Caller
from test_emitters_cpu import emitter_scene, materials, random_tris, world_tris
from test_hemisphere_gpu import DEV, Dev, hit_point
from test_lighting_gpu import environment
from test_surface_gpu import words

pytestmark = pytest.mark.gpu

F = np.float32
FAR = F(1e30)
FRAME = 5
GRID = (100, 37)            # 12 whole tiles and a clipped column and row of them; 3 700 records: the plain kernels
BAND = (5, 29)
PLAIN = {"room": "trace_emitter_shadow_lane_kernel<", "room_tl": "trace_emitter_shadow_two_level_kernel<", "soup": "trace_emitter_shadow_lane_kernel<"}
ORACLES = {}


class World:
    """One context with an emitter scene uploaded (flat, or two-level for room_tl), its shade data and emitter table resident."""

    def __init__(self, kind):
        self.kind = kind
        self.verts, self.layers, self.cam_def, self.shade = emitter_scene(kind)
        self.tris = world_tris(self.verts, self.layers)
        self.ctx = capi.Context(0)
        self.dev = Dev(self.ctx)
        if kind == "room_tl":
            from messyerraytracer_amd import synth
            self.ctx.upload_two_level_scene(*synth.room())
        else:
            nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(self.verts))
            self.ctx.upload_scene(capi.make_triangles(self.verts, layers=self.layers), nodes, prim_idx)
        self.ctx.upload_shade_data(self.shade.n_tris, self.shade.materials, self.shade.material_ids)
        self.table = E.build_table(self.tris, self.shade)
        assert self.ctx.build_emitters(self.tris) == (self.table[0].shape[0], int(self.table[1][-1]))

    def oracle(self):
        if self.kind not in ORACLES:
            ORACLES[self.kind] = po.OracleScene(self.verts, layers=self.layers)
        return ORACLES[self.kind]

    def walk(self):
        """the oracle's walk of the scene as uploaded: the two-level walk for room_tl (brute force is over the flattened triangles)"""
        if self.kind != "room_tl":
            return self.oracle()
        if "tl_walk" not in ORACLES:
            from messyerraytracer_amd import synth
            ORACLES["tl_walk"] = po.OracleTwoLevelScene(*synth.room())
        return ORACLES["tl_walk"]

    def camera(self, w, h):
        return capi.camera_look(self.cam_def[0], self.cam_def[1], w, h, self.cam_def[2])

    def grid_rays(self, w, h, y0=0, y1=None):
        return po.grid_rays(self.cam_def[0], self.cam_def[1], w, h, self.cam_def[2], y0, y1)

    def close(self):
        self.dev.free()
        self.ctx.close()


def check_cast(wd, emitter, mask, sample, query_mask=0xFFFFFFFF, what=""):
    """The words against the restatement; the mask bytes against the oracle's any-hit of the restatement's rays, computed by the walk and
    by brute force: records on which the two disagree are left out, at most 1 % of them."""
    np.testing.assert_array_equal(emitter, sample["emitter"], err_msg=what + ": d_out_emitter")
    a = wd.walk().trace(sample["rays"], query_mask=query_mask, any_hit=True)["prim_id"] >= 0
    b = wd.oracle().brute(sample["rays"], query_mask=query_mask, any_hit=True)["prim_id"] >= 0
    agree = a == b
    assert (~agree).sum() <= 0.01 * agree.shape[0], (what, (~agree).sum())
    want = (~(sample["traced"] & a)).astype(np.uint8)
    np.testing.assert_array_equal(mask[agree], want[agree], err_msg=what + ": d_mask against the oracle")
    assert (mask[~sample["traced"]] == 1).all(), what


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tris", [1, 2, 63, 64, 65, 257, 1025, 11076])
def test_table_equals_numpy_word_for_word(built, n_tris):
    """None, one, every third and all triangles emissive (materials 1 and 2 in turn), from host arrays and from device arrays."""
    tris = random_tris(n_tris, seed=n_tris)
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        d_tris = dev.put(tris)
        k = np.arange(n_tris, dtype=np.uint32)
        patterns = dict(none=np.zeros(n_tris, np.uint32), one=np.where(k == n_tris // 2, 2, 0), third=np.where(k % 3 == 1, 1 + (k // 3) % 2, 0),
                        all=1 + k % 2)
        assert ctx.build_emitters(tris) == (0, 0)                                       # no shade data resident
        for name, ids in patterns.items():
            shade = S.ShadeData(n_tris, materials(), ids.astype(np.uint32))
            ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids)
            rows, cdf = E.build_table(tris, shade)
            for on_device in (False, True):
                ctx.clear_emitters()
                assert ctx.emitter_info() == (0, 0)
                got = ctx.build_emitters(d_tris, n_tris, on_device=True) if on_device else ctx.build_emitters(tris)
                assert got == (rows.shape[0], int(cdf[-1]) if len(cdf) else 0), (name, on_device)
                g_rows, g_cdf = ctx.emitter_table()
                np.testing.assert_array_equal(words(g_rows), words(rows), err_msg=f"{name}: rows")
                np.testing.assert_array_equal(g_cdf, cdf, err_msg=f"{name}: cdf")
            assert rows.shape[0] == dict(none=0, one=1, third=(n_tris + 1) // 3, all=n_tris)[name]
    finally:
        dev.free()
        ctx.close()


def test_table_leaves_out_what_cannot_emit_and_survives_a_scene_upload(built):
    """Zero area, ids out of range, an energy <= 0, weights that are not finite; the table is the context's: a scene upload leaves it."""
    n = 300
    tris = random_tris(n, seed=8)
    ids = 1 + np.arange(n, dtype=np.uint32) % 2
    tris["edge2"][3] = tris["edge1"][3] * F(2)
    tris["edge1"][4] = 0
    tris["id"][5], tris["id"][6] = n, 0xFFFFFFFF
    ids[7], ids[8], ids[9] = 4, 0, 3
    tris["edge1"][10] = F(3e38)
    tris["edge1"][11, 0] = np.nan
    tris["id"][[0, 8]] = 8, 0
    shade = S.ShadeData(n, materials(), ids)
    rows, cdf = E.build_table(tris, shade)
    assert rows.shape[0] == n - 9
    wd = World("soup")
    try:
        ctx = wd.ctx
        ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids)
        assert ctx.build_emitters(tris) == (n - 9, int(cdf[-1]))
        for again in range(2):
            g_rows, g_cdf = ctx.emitter_table()
            np.testing.assert_array_equal(words(g_rows), words(rows))
            np.testing.assert_array_equal(g_cdf, cdf)
            nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(wd.verts))
            ctx.upload_scene(capi.make_triangles(wd.verts, layers=wd.layers), nodes, prim_idx)
        ctx.upload_shade_data(n, None, ids)                                              # ids without materials: nothing can emit
        assert ctx.build_emitters(tris) == (0, 0) and ctx.emitter_table()[0].shape[0] == 0
    finally:
        wd.close()


def test_too_many_emitters_are_refused_and_the_old_table_answers(built):
    n = T.MAX_EMITTERS + 1
    rng = np.random.default_rng(3)
    tris = np.zeros(n, T.TRI64)
    tris["v0"], tris["edge1"], tris["edge2"] = rng.uniform(-4, 4, (n, 3)), rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-0.5, 0.5, (n, 3))
    tris["id"] = np.arange(n)
    ctx = capi.Context(0)
    try:
        ctx.upload_shade_data(n, materials(), np.ones(n, np.uint32))
        old = E.build_table(tris[:1000], S.ShadeData(n, materials(), np.ones(n, np.uint32)))
        assert ctx.build_emitters(tris[:1000]) == (1000, int(old[1][-1]))
        with pytest.raises(capi.MrtError) as err:
            ctx.build_emitters(tris)
        assert err.value.status == capi.ERR_UNSUPPORTED and "MRT_MAX_EMITTERS" in str(err.value)
        assert ctx.emitter_info() == (1000, int(old[1][-1]))
        g_rows, g_cdf = ctx.emitter_table()
        np.testing.assert_array_equal(words(g_rows), words(old[0]))
        np.testing.assert_array_equal(g_cdf, old[1])
        # exactly MRT_MAX_EMITTERS is a table: equal weights would not tell much, so every q and the total are checked
        rows, cdf = E.build_table(tris[:-1], S.ShadeData(n, materials(), np.ones(n, np.uint32)))
        assert ctx.build_emitters(tris[:-1]) == (T.MAX_EMITTERS, int(cdf[-1]))
        g_rows, g_cdf = ctx.emitter_table()
        np.testing.assert_array_equal(g_rows["q"], rows["q"])
        np.testing.assert_array_equal(g_cdf, cdf)
    finally:
        ctx.close()


# ---- the cast ----------------------------------------------------------------------------------------------------------------------------

def grid_form(wd, y0, y1, draw):
    w, h = GRID
    ctx, dev = wd.ctx, wd.dev
    cam = wd.camera(w, h)
    n = w * (y1 - y0)
    rays = wd.grid_rays(w, h, y0, y1)
    d_hits = dev.alloc(n * 32)
    ctx.cast_grid(cam, w, h, y0=y0, y1=y1, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
    hits = dev.get(d_hits, n, T.HIT32)
    d_mask, d_em = dev.put(np.full(n + 64, 0x5A, np.uint8)), dev.put(np.full(n + 16, 0x5A5A5A5A, np.uint32))
    ctx.cast_grid_emitter_shadows(cam, w, h, d_hits, d_mask, d_em, FRAME, draw, y0=y0, y1=y1)
    assert ctx.last_kernel_variant().startswith(PLAIN[wd.kind]), ctx.last_kernel_variant()
    mask, em = dev.get(d_mask, n + 64, np.uint8), dev.get(d_em, n + 16, np.uint32)
    assert (mask[n:] == 0x5A).all() and (em[n:] == 0x5A5A5A5A).all()                    # nothing behind the last record
    pixel = np.arange(n, dtype=np.uint64) + y0 * w                                       # the whole grid's index
    hit = hits["prim_id"] != -1
    s = E.emitter_samples(rays["direction"], hit_point(rays, hits), hits["normal"], hit, pixel, FRAME, draw, *wd.table)
    check_cast(wd, em[:n], mask[:n], s, what=f"{wd.kind} grid rows {y0}..{y1}")
    return em[:n], mask[:n], s


@pytest.mark.parametrize("kind", ["room", "room_tl", "soup"])
def test_grid_and_band_against_the_restatement_and_the_oracle(built, kind):
    """Grid 100 x 37 whole, and its rows [5, 29): the band samples, and shadows, what the whole frame does."""
    wd = World(kind)
    try:
        draw = T.path_emitter_draw(1)
        whole = grid_form(wd, 0, GRID[1], draw)
        band = grid_form(wd, BAND[0], BAND[1], draw)
        a, b = BAND[0] * GRID[0], BAND[1] * GRID[0]
        np.testing.assert_array_equal(whole[0][a:b], band[0])
        np.testing.assert_array_equal(whole[1][a:b], band[1])
        s = whole[2]
        on = s["emitter"] != T.EMITTER_NONE
        assert len(np.unique(s["emitter"][on])) > 50 and (whole[1] == 0).any() and (s["traced"] & (whole[1] == 1)).any()
        assert (on & ~s["traced"]).any()                                                 # refusals occur
    finally:
        wd.close()


@pytest.mark.parametrize("kind", ["room", "room_tl", "soup"])
def test_array_forms_in_both_layouts(built, kind):
    """1, 63, 65 and 4096 records of a 64 x 64 grid as arrays on the plain kernels, in the packed and in the reference's host layout;
    the 4096 tiled to 65 536 records on the persistent kernels."""
    wd = World(kind)
    ctx, dev = wd.ctx, wd.dev
    try:
        rays = wd.grid_rays(64, 64)
        hrays = po.make_host_rays(rays)
        d_rays, d_hr = dev.put(rays), dev.put(hrays)
        d_h32, d_h44 = dev.alloc(4096 * 32), dev.alloc(4096 * 44)
        ctx.cast(d_rays, d_h32, count=4096, flags=DEV)
        ctx.cast(d_hr, d_h44, count=4096, flags=DEV | capi.FLAG_HOST_LAYOUT)
        hits, h44 = dev.get(d_h32, 4096, T.HIT32), dev.get(d_h44, 4096, T.HOST_HIT44)
        pos = hit_point(rays, hits)
        d_mask, d_em = dev.alloc(65536), dev.alloc(65536 * 4)
        for i, n in enumerate((1, 63, 65, 4096)):
            draw = T.path_emitter_draw(i)
            pixel = np.arange(n, dtype=np.uint64)                                        # the array form: the record's index
            ctx.cast_emitter_shadows(d_rays, d_h32, n, d_mask, d_em, FRAME, draw)
            assert ctx.last_kernel_variant().startswith(PLAIN[kind]), ctx.last_kernel_variant()
            s = E.emitter_samples(rays["direction"][:n], pos[:n], hits["normal"][:n], hits["prim_id"][:n] != -1, pixel, FRAME, draw, *wd.table)
            check_cast(wd, dev.get(d_em, n, np.uint32), dev.get(d_mask, n, np.uint8), s, what=f"{kind} ray32 {n}")
            ctx.cast_emitter_shadows(d_hr, d_h44, n, d_mask, d_em, FRAME, draw, flags=capi.FLAG_HOST_LAYOUT)
            assert ctx.last_kernel_variant().startswith(PLAIN[kind]), ctx.last_kernel_variant()
            s = E.emitter_samples(hrays["direction"][:n], h44["position"][:n], h44["normal"][:n], h44["prim_id"][:n] != T.NO_HIT, pixel, FRAME, draw, *wd.table)
            check_cast(wd, dev.get(d_em, n, np.uint32), dev.get(d_mask, n, np.uint8), s, what=f"{kind} host layout {n}")
        # 16 copies of the records: the same surfaces under 65 536 different streams
        big_rays, big_hits = np.tile(rays, 16), np.tile(hits, 16)
        d_br, d_bh = dev.put(big_rays), dev.put(big_hits)
        draw = T.path_emitter_draw(2)
        ctx.cast_emitter_shadows(d_br, d_bh, 65536, d_mask, d_em, FRAME, draw)
        assert "emitter_shadow_persistent" in ctx.last_kernel_variant(), ctx.last_kernel_variant()
        s = E.emitter_samples(big_rays["direction"], np.tile(pos, (16, 1)), big_hits["normal"], big_hits["prim_id"] != -1,
                              np.arange(65536, dtype=np.uint64), FRAME, draw, *wd.table)
        check_cast(wd, dev.get(d_em, 65536, np.uint32), dev.get(d_mask, 65536, np.uint8), s, what=f"{kind} persistent")
    finally:
        wd.close()


@pytest.mark.parametrize("kind", ["soup", "room"])
def test_select_bytes_misses_query_mask_and_an_empty_table(built, kind):
    """A d_select with zeros and (the soup) misses among the records: MRT_EMITTER_NONE, lit.  A query_mask that hides the occluders (the
    room's sphere and boxes, layer 1: inside a closed room it is they that shadow the ceiling's light): the same words, the oracle's bytes
    under that mask.  An empty table: every word MRT_EMITTER_NONE, every byte 1."""
    wd = World(kind)
    ctx, dev = wd.ctx, wd.dev
    try:
        w, h = GRID
        n = w * h
        cam, rays = wd.camera(w, h), wd.grid_rays(w, h)
        d_hits = dev.alloc(n * 32)
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        hits = dev.get(d_hits, n, T.HIT32)
        hit = hits["prim_id"] != -1
        assert kind != "soup" or (~hit).any()
        select = (np.arange(n) % 3 != 1).astype(np.uint8)
        d_sel, d_mask, d_em = dev.put(select), dev.alloc(n), dev.alloc(n * 4)
        draw = T.path_emitter_draw(3)
        s = E.emitter_samples(rays["direction"], hit_point(rays, hits), hits["normal"], hit, np.arange(n, dtype=np.uint64), FRAME, draw, *wd.table, select)
        full = None
        for qm in (0xFFFFFFFF, 2):
            ctx.cast_grid_emitter_shadows(cam, w, h, d_hits, d_mask, d_em, FRAME, draw, d_select=d_sel, query_mask=qm)
            em, mask = dev.get(d_em, n, np.uint32), dev.get(d_mask, n, np.uint8)
            check_cast(wd, em, mask, s, qm, what=f"query_mask {qm}")
            assert (em[select == 0] == T.EMITTER_NONE).all() and (em[~hit] == T.EMITTER_NONE).all()
            assert (em[hit & (select != 0)] != T.EMITTER_NONE).mean() > 0.99
            if qm == 2:
                assert kind == "soup" or ((mask == 1) & (full == 0)).any()               # the sphere and the boxes no longer shadow
            full = mask
        ctx.clear_emitters()
        ctx.cast_grid_emitter_shadows(cam, w, h, d_hits, d_mask, d_em, FRAME, draw)
        assert (dev.get(d_em, n, np.uint32) == T.EMITTER_NONE).all() and (dev.get(d_mask, n, np.uint8) == 1).all()
        d_out = dev.put(np.full(n * 4, -7.5, F))
        d_rows = dev.alloc(n * 64)
        ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows)
        ctx.light_grid_emitter_surfaces(cam, w, h, d_hits, d_rows, d_em, d_out, d_mask, FRAME, draw)
        out = dev.get(d_out, n * 4, F).reshape(-1, 4)
        assert (out[hit] == (0, 0, 0, 1)).all() and (out[~hit] == 0).all()
    finally:
        wd.close()


# ---- the light call and the step -----------------------------------------------------------------------------------------------------------

class Lit:
    """A World with the primary grid cast, its rows and shading-normal records resolved and the emitter cast of bounce 0 made."""

    def __init__(self, kind, w, h, draw):
        self.wd = wd = World(kind)
        ctx, dev = wd.ctx, wd.dev
        self.w, self.h, self.n, self.draw = w, h, w * h, draw
        n = self.n
        self.cam, self.rays = wd.camera(w, h), wd.grid_rays(w, h)
        self.d_hits, self.d_rows, self.d_pairs, self.d_shits = dev.alloc(n * 32), dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 32)
        ctx.cast_grid(self.cam, w, h, hits=self.d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        ctx.resolve_grid_surfaces(self.cam, w, h, self.d_hits, self.d_rows, self.d_pairs, self.d_shits)
        self.hits, self.shits, self.rows = dev.get(self.d_hits, n, T.HIT32), dev.get(self.d_shits, n, T.HIT32), dev.get(self.d_rows, n, T.SURFACE64)
        self.hit = self.hits["prim_id"] != -1
        self.pos = hit_point(self.rays, self.hits)
        self.pixel = np.arange(n, dtype=np.uint64)
        self.d_mask, self.d_em = dev.alloc(n), dev.alloc(n * 4)
        ctx.cast_grid_emitter_shadows(self.cam, w, h, self.d_shits, self.d_mask, self.d_em, FRAME, draw)
        self.mask, self.em = dev.get(self.d_mask, n, np.uint8), dev.get(self.d_em, n, np.uint32)
        self.sample = E.emitter_samples(self.rays["direction"], self.pos, self.shits["normal"], self.hit, self.pixel, FRAME, draw, *wd.table)
        np.testing.assert_array_equal(self.em, self.sample["emitter"])

    def close(self):
        self.wd.close()


@pytest.mark.parametrize("kind", ["room", "soup"])
def test_light_call_matches_the_restatement(built, kind):
    """Rows resolved from the scene: the grid form, the array form and the host-layout array form against emitters.emitter_direct with
    the words and bytes the cast wrote; with and without the mask; written and accumulated."""
    lit = Lit(kind, *GRID, T.path_emitter_draw(0))
    ctx, dev, n = lit.wd.ctx, lit.wd.dev, lit.n
    try:
        base = np.random.default_rng(4).uniform(0, 2, (n, 4)).astype(F)
        d_rays = dev.put(lit.rays)
        for m, dm in ((lit.mask, lit.d_mask), (None, None)):
            for b in (None, base):
                want = E.emitter_direct(lit.rows, lit.hit, lit.sample, m, b)
                d_out = dev.put(np.concatenate([(np.full((n, 4), -7.5, F) if b is None else b).reshape(-1), np.full(64, -7.5, F)]))
                ctx.light_grid_emitter_surfaces(lit.cam, lit.w, lit.h, lit.d_shits, lit.d_rows, lit.d_em, d_out, dm, FRAME, lit.draw, accumulate=b is not None)
                got = dev.get(d_out, n * 4 + 64, F)
                np.testing.assert_array_equal(words(got[:n * 4].reshape(-1, 4)), words(want), err_msg="grid form")
                assert (got[n * 4:] == F(-7.5)).all()
                if b is not None:
                    ctx.h2d(d_out, b)
                ctx.light_emitter_surfaces(d_rays, lit.d_shits, lit.d_rows, n, lit.d_em, d_out, dm, FRAME, lit.draw, accumulate=b is not None)
                np.testing.assert_array_equal(words(dev.get(d_out, n * 4, F).reshape(-1, 4)), words(want), err_msg="array form")
        bare = E.emitter_direct(lit.rows, lit.hit, lit.sample, lit.mask)
        assert np.isfinite(bare).all() and (bare[lit.hit, :3] > 0).any() and (bare[lit.hit & (lit.mask == 0), :3] == 0).all()
        assert (lit.mask == 0).any()
        # the reference's host layout
        hrays = po.make_host_rays(lit.rays)
        d_hr, d_h44, d_rows44, d_s44 = dev.put(hrays), dev.alloc(n * 44), dev.alloc(n * 64), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        ctx.resolve_surfaces(d_hr, d_h44, n, d_rows44, None, d_s44, flags=capi.FLAG_HOST_LAYOUT)
        ctx.cast_emitter_shadows(d_hr, d_s44, n, lit.d_mask, lit.d_em, FRAME, lit.draw, flags=capi.FLAG_HOST_LAYOUT)
        s44, rows44 = dev.get(d_s44, n, T.HOST_HIT44), dev.get(d_rows44, n, T.SURFACE64)
        mask = dev.get(lit.d_mask, n, np.uint8)
        hit44 = s44["prim_id"] != T.NO_HIT
        s = E.emitter_samples(hrays["direction"], s44["position"], s44["normal"], hit44, lit.pixel, FRAME, lit.draw, *lit.wd.table)
        np.testing.assert_array_equal(dev.get(lit.d_em, n, np.uint32), s["emitter"])
        d_out = dev.alloc(n * 16)
        ctx.light_emitter_surfaces(d_hr, d_s44, d_rows44, n, lit.d_em, d_out, lit.d_mask, FRAME, lit.draw, flags=capi.FLAG_HOST_LAYOUT)
        np.testing.assert_array_equal(words(dev.get(d_out, n * 4, F).reshape(-1, 4)), words(E.emitter_direct(rows44, hit44, s, mask)), err_msg="host layout")
    finally:
        lit.close()


def edge_records():
    """Hand-made records around one tiny emitter at the origin (edges of 1e-7 in the plane y = 0, so that every sampled point is the
    origin to within 1e-7 and has y = 0 exactly) that put dist, n . dir and |ng . dir| on both sides of their thresholds, and at
    n . dir = 0 exactly.  Returns (tris, rays, hits, rows)."""
    tri = np.zeros(1, T.TRI64)
    tri["edge1"], tri["edge2"] = (1e-7, 0, 0), (0, 0, 1e-7)
    p, nrm = [], []
    for delta in (0.25e-6, 0.5e-6, 0.9e-6, 1.1e-6, 2e-6, 4e-6, 1e-5):                   # org = -n * delta: dist about delta, dir = n
        for n in ((0, -1, 0), (0.6, -0.8, 0)):
            n = np.array(n)
            p.append(-n * (delta + 1e-3))                                                # (the kernel adds n * 1e-3 to p)
            nrm.append(n)
    to = np.array([-1.0, -0.5, 0.0]) / np.sqrt(1.25)                                      # from org = (1, 0.5, 0) to the emitter: seen at 27 degrees
    for tilt in (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5):                            # n . dir about tilt
        n = np.array([-0.5, 1.0, 0.0]) / np.sqrt(1.25) + tilt * to
        n /= np.linalg.norm(n)
        p.append(np.array([1.0, 0.5, 0.0]) - n * 1e-3)
        nrm.append(n)
    p.append(np.array([1.0, -1e-3, 0.0]))                                                # org.y = -1e-3 + 1e-3 = 0 exactly: n . dir = 0
    nrm.append(np.array([0.0, 1.0, 0.0]))
    for hgt in (0.25e-6, 0.5e-6, 0.9e-6, 1.1e-6, 2e-6, 4e-6, 1e-5, -0.9e-6, -1.1e-6):    # |ng . dir| about |hgt|, n = (-1, 0, 0)
        n = np.array([-1.0, 0.0, 0.0])
        p.append(np.array([1.0, hgt, 0.0]) - n * 1e-3)
        nrm.append(n)
    p, nrm = np.array(p, F), np.array(nrm, F)
    m = p.shape[0]
    reps = 19                                                                            # 19 streams per record: 589 records, three workgroups
    p, nrm = np.tile(p, (reps, 1)), np.tile(nrm, (reps, 1))
    n = p.shape[0]
    d = (-nrm).astype(F)                                                                  # the incoming ray arrives along -n: the normal is not turned
    rays = np.zeros(n, T.RAY32)
    rays["direction"], rays["origin"], rays["t_max"] = d, p, FAR                         # t = 0: the record's position is p exactly
    hits = np.zeros(n, T.HIT32)
    hits["t"], hits["prim_id"], hits["normal"] = 0, np.arange(n), nrm
    rows = np.zeros(n, T.SURFACE64)
    rows["normal"], rows["n_dot_v"], rows["albedo"], rows["metallic"], rows["roughness"], rows["specular"] = nrm, 1, (0.8, 0.6, 0.4), 0.25, 0.5, 0.5
    return tri, rays, hits, rows, m


def test_light_call_at_the_refusal_edges(built):
    """Each of the three refusals occurs and does not occur next to its threshold; the device agrees with the restatement word for word."""
    tri, rays, hits, rows, m = edge_records()
    n = rays.shape[0]
    shade = S.ShadeData(1, materials(), np.array([1], np.uint32))
    table = E.build_table(tri, shade)
    assert table[0].shape[0] == 1 and table[0]["area"][0] > 0
    pos = hit_point(rays, hits)
    hit = np.ones(n, bool)
    pixel = np.arange(n, dtype=np.uint64)
    draw = T.path_emitter_draw(4)
    s = E.emitter_samples(rays["direction"], pos, hits["normal"], hit, pixel, FRAME, draw, *table)
    assert (s["emitter"] == 0).all()
    with np.errstate(all="ignore"):
        dist = np.sqrt(s["dist2"])
    near, away, edge_on = dist < F(1e-6), ~(dist < F(1e-6)) & (s["ndl"] <= 0), ~(dist < F(1e-6)) & ~(s["ndl"] <= 0) & (s["cy"] < F(1e-6))
    kinds = np.arange(n) % m
    for name, refused, group in (("dist", near, kinds < 14), ("ndl", away, (kinds >= 14) & (kinds < 22)), ("cy", edge_on, kinds >= 22)):
        assert refused[group].any() and (s["traced"] & group).any(), name
        assert not (refused & ~group).any(), name                                        # each group meets its own refusal alone
    assert (s["ndl"][kinds == 21] == 0).all() and not s["traced"][kinds == 21].any()      # n . dir = 0 exactly: refused
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        ctx.upload_shade_data(1, shade.materials, shade.material_ids)
        assert ctx.build_emitters(tri)[0] == 1
        d_rays, d_hits, d_rows = dev.put(rays), dev.put(hits), dev.put(rows)
        d_em, d_out = dev.put(np.zeros(n, np.uint32)), dev.put(np.full(n * 4 + 64, -7.5, F))
        ctx.light_emitter_surfaces(d_rays, d_hits, d_rows, n, d_em, d_out, None, FRAME, draw)
        got = dev.get(d_out, n * 4 + 64, F)
        want = E.emitter_direct(rows, hit, s)
        np.testing.assert_array_equal(words(got[:n * 4].reshape(-1, 4)), words(want))
        assert (got[n * 4:] == F(-7.5)).all()
        assert ((want[:, :3] > 0).all(axis=1) == s["traced"]).all()
        # a word past the table is no emitter
        ctx.h2d(d_em, np.where(np.arange(n) % 2 == 0, 1, T.EMITTER_NONE).astype(np.uint32))
        ctx.light_emitter_surfaces(d_rays, d_hits, d_rows, n, d_em, d_out, None, FRAME, draw)
        assert (dev.get(d_out, n * 4, F).reshape(-1, 4) == (0, 0, 0, 1)).all()
    finally:
        dev.free()
        ctx.close()


@pytest.mark.parametrize("kind", ["room", "soup"])
def test_emitter_step_against_the_step_and_the_restatement(built, kind):
    """Bounces 0, 1 and 3 on the grid's records with a random state: with every d_prev_lobe MRT_LOBE_SPECULAR the output is mrt_path_step's
    word for word; with every one MRT_LOBE_DIFFUSE the radiance differs exactly by t * emission on the emissive hits, from bounce 1 on;
    a mixed array against emitters.path_step_emitters; the grid and the array form; d_prev_lobe = d_out_lobe."""
    lit = Lit(kind, *GRID, T.path_emitter_draw(0))
    ctx, dev, n = lit.wd.ctx, lit.wd.dev, lit.n
    try:
        rng = np.random.default_rng(7)
        state0 = P.init_state(n)
        state0["throughput"], state0["radiance"] = rng.uniform(0.1, 1.0, (n, 3)), rng.uniform(0.0, 0.5, (n, 3))
        state0["active"] = rng.random(n) < 0.9
        direct = E.emitter_direct(lit.rows, lit.hit, lit.sample, lit.mask)
        env = environment()
        d_direct, d_state, d_sel, d_lobe, d_prev, d_rays = dev.put(direct), dev.alloc(n * 32), dev.alloc(n), dev.alloc(n), dev.alloc(n), dev.put(lit.rays)
        emissive = lit.hit & (lit.rows["emission"] > 0).any(axis=1) & (state0["active"] != 0)
        assert emissive.sum() > 20
        mixed = rng.integers(0, 3, n).astype(np.uint8)

        def run(bounce, prev, grid=True, same_array=False):
            ctx.h2d(d_state, state0)
            kw = dict(frame=FRAME, bounce=bounce, max_bounces=3, d_out_lobe=d_prev if same_array else d_lobe)
            if prev is not None:
                ctx.h2d(d_prev, prev)
            if prev is False:                                                            # mrt_path_step itself
                if grid:
                    ctx.path_grid_step(lit.cam, lit.w, lit.h, lit.d_shits, lit.d_rows, d_direct, d_state, env, d_sel, **kw)
                else:
                    ctx.path_step(d_rays, lit.d_shits, lit.d_rows, n, d_direct, d_state, env, d_sel, **kw)
            elif grid:
                ctx.path_grid_step_emitters(lit.cam, lit.w, lit.h, lit.d_shits, lit.d_rows, d_direct, d_state, env, d_sel, None if prev is None else d_prev, **kw)
            else:
                ctx.path_step_emitters(d_rays, lit.d_shits, lit.d_rows, n, d_direct, d_state, env, d_sel, None if prev is None else d_prev, **kw)
            return dev.get(d_state, n, T.PATH_STATE), dev.get(d_sel, n, np.uint8), dev.get(d_prev if same_array else d_lobe, n, np.uint8)

        for bounce in (0, 1, 3):
            plain = run(bounce, False)
            want = P.path_step(state0, lit.rows, lit.hit, lit.shits["normal"], lit.rays["direction"], direct, env, lit.pixel, FRAME, bounce, 3)
            np.testing.assert_array_equal(words(plain[0]), words(want[0]))
            spec = run(bounce, np.full(n, B.LOBE_SPECULAR, np.uint8))
            np.testing.assert_array_equal(words(spec[0]), words(plain[0]))
            np.testing.assert_array_equal(spec[1], plain[1])
            np.testing.assert_array_equal(spec[2], plain[2])
            diffuse = run(bounce, np.full(n, B.LOBE_DIFFUSE, np.uint8))
            if bounce == 0:                                                              # the emission line always runs, with or without lobe bytes
                np.testing.assert_array_equal(words(diffuse[0]), words(plain[0]))
                np.testing.assert_array_equal(words(run(0, None)[0]), words(plain[0]))
            else:
                changed = (words(diffuse[0]).reshape(n, 8) != words(plain[0]).reshape(n, 8)).any(axis=1)
                assert not (changed & ~emissive).any() and changed[emissive].mean() > 0.9
                np.testing.assert_array_equal(diffuse[0]["throughput"], plain[0]["throughput"])
                np.testing.assert_array_equal(diffuse[1], plain[1])
                w_ = E.path_step_emitters(state0, lit.rows, lit.hit, lit.shits["normal"], lit.rays["direction"], direct, env, lit.pixel, FRAME, bounce, 3,
                                          np.full(n, B.LOBE_DIFFUSE, np.uint8))
                np.testing.assert_array_equal(words(diffuse[0]), words(w_[0]))
                # exactly t * emission: the restatement's radiance without the line, then the line's own addend in the step's order
                t, em = state0["throughput"][emissive], lit.rows["emission"][emissive]
                r_with = ((state0["radiance"][emissive] + t * em) + t * direct[emissive, :3]).astype(F)
                r_without = (state0["radiance"][emissive] + t * direct[emissive, :3]).astype(F)
                np.testing.assert_array_equal(plain[0]["radiance"][emissive], r_with)
                np.testing.assert_array_equal(diffuse[0]["radiance"][emissive], r_without)
            for grid in (True, False):
                for same_array in (False, True):
                    got = run(bounce, mixed, grid, same_array)
                    want = E.path_step_emitters(state0, lit.rows, lit.hit, lit.shits["normal"], lit.rays["direction"], direct, env, lit.pixel, FRAME,
                                                bounce, 3, mixed)
                    np.testing.assert_array_equal(words(got[0]), words(want[0]), err_msg=f"bounce {bounce} grid {grid} same array {same_array}")
                    np.testing.assert_array_equal(got[1], want[1])
                    np.testing.assert_array_equal(got[2], want[2])
    finally:
        lit.close()


def test_whole_frame_against_the_numpy_loop(built):
    """Grid 32 x 24 of the room, max_bounces = 3, no analytic light: per bounce cast -> resolve -> emitter shadows -> emitter light ->
    emitter step -> bounce cast, every call ASYNC (the last bounce without the emitter pair); every state word, word and byte against
    the restatements fed with the device's records."""
    w, h, bounces = 32, 24, 3
    lit = Lit("room", w, h, T.path_emitter_draw(0))
    wd = lit.wd
    ctx, dev, n = wd.ctx, wd.dev, lit.n
    A = capi.FLAG_ASYNC
    try:
        env = environment()
        pairs = [(dev.alloc(n * 32), dev.alloc(n * 32)), (dev.alloc(n * 32), dev.alloc(n * 32))]
        d_rows, d_pairs, d_shits, d_mask, d_em, d_direct = dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 32), dev.alloc(n), dev.alloc(n * 4), dev.alloc(n * 16)
        d_state, d_select, d_lobe = dev.alloc(n * 32), dev.alloc(n), dev.alloc(n)
        d_counts = dev.put(np.zeros(bounces + 1, np.uint32))
        zeros = np.zeros((n, 4), F)
        ctx.path_init(d_state, n, flags=A)
        state = P.init_state(n)
        pixel = lit.pixel
        rays_host = lit.rays
        select, lobe = None, None
        lit_records = 0
        for b in range(bounces + 1):
            cur_rays, cur_hits = (None, lit.d_hits) if b == 0 else pairs[b & 1]
            nxt_rays, nxt_hits = pairs[(b + 1) & 1]
            draw = T.path_emitter_draw(b)
            kw = dict(frame=FRAME, bounce=b, max_bounces=bounces, d_out_lobe=d_lobe, d_active_count=d_counts + 4 * b, flags=A)
            sample_emitters = b < bounces
            if not sample_emitters:
                ctx.h2d(d_direct, zeros)
            if b == 0:
                ctx.resolve_grid_surfaces(lit.cam, w, h, cur_hits, d_rows, d_pairs, d_shits, flags=A)
                if sample_emitters:
                    ctx.cast_grid_emitter_shadows(lit.cam, w, h, d_shits, d_mask, d_em, FRAME, draw, flags=A)
                    ctx.light_grid_emitter_surfaces(lit.cam, w, h, d_shits, d_rows, d_em, d_direct, d_mask, FRAME, draw, flags=A)
                ctx.path_grid_step_emitters(lit.cam, w, h, d_shits, d_rows, d_direct, d_state, env, d_select, None, **kw)
            else:
                ctx.resolve_surfaces(cur_rays, cur_hits, n, d_rows, d_pairs, d_shits, flags=A)
                if sample_emitters:
                    ctx.cast_emitter_shadows(cur_rays, d_shits, n, d_mask, d_em, FRAME, draw, d_select=d_select, flags=A)
                    ctx.light_emitter_surfaces(cur_rays, d_shits, d_rows, n, d_em, d_direct, d_mask, FRAME, draw, flags=A)
                ctx.path_step_emitters(cur_rays, d_shits, d_rows, n, d_direct, d_state, env, d_select, d_lobe, **kw)   # (d_prev_lobe = d_out_lobe)
            if b < bounces:
                bk = dict(frame=FRAME, first_draw=P.first_draw(b), t_max=FAR, d_select=d_select, d_surface=d_pairs, d_out_rays=nxt_rays, flags=A)
                if b == 0:
                    ctx.cast_grid_bounce(lit.cam, w, h, d_shits, nxt_hits, **bk)
                else:
                    ctx.cast_bounce(cur_rays, d_shits, n, nxt_hits, **bk)
            ctx.synchronize()
            # the same bounce in numpy, on the device's records
            hits, shits, rows = dev.get(cur_hits, n, T.HIT32), dev.get(d_shits, n, T.HIT32), dev.get(d_rows, n, T.SURFACE64)
            hit = hits["prim_id"] != -1
            direct = zeros
            if sample_emitters:
                s = E.emitter_samples(rays_host["direction"], hit_point(rays_host, hits), shits["normal"], hit, pixel, FRAME, draw, *wd.table, select)
                np.testing.assert_array_equal(dev.get(d_em, n, np.uint32), s["emitter"], err_msg=f"emitter words of bounce {b}")
                mask = dev.get(d_mask, n, np.uint8)
                assert (mask[~s["traced"]] == 1).all()
                lit_records += int((s["traced"] & (mask == 1)).sum())
                direct = E.emitter_direct(rows, hit, s, mask)
                np.testing.assert_array_equal(words(dev.get(d_direct, n * 4, F).reshape(-1, 4)), words(direct), err_msg=f"direct of bounce {b}")
            state, select, lobe, count = E.path_step_emitters(state, rows, hit, shits["normal"], rays_host["direction"], direct, env, pixel, FRAME, b,
                                                              bounces, lobe)
            np.testing.assert_array_equal(words(dev.get(d_state, n, T.PATH_STATE)).reshape(-1, 8), words(state).reshape(-1, 8), err_msg=f"state after bounce {b}")
            np.testing.assert_array_equal(dev.get(d_select, n, np.uint8), select)
            np.testing.assert_array_equal(dev.get(d_lobe, n, np.uint8), lobe)
            assert int(dev.get(d_counts + 4 * b, 1, np.uint32)[0]) == count
            if b < bounces:
                rays_host = dev.get(nxt_rays, n, T.RAY32)
            if count == 0:
                break
        assert b == bounces and lit_records > n // 4                                        # (the loop ends early only when nothing is active)
        assert (state["active"] == 0).all() and (state["radiance"] > 0).any() and np.isfinite(state["radiance"]).all()
    finally:
        lit.close()


# ---- the interface ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_in_the_stated_order_and_empty_calls(built):
    """Every MRT_ERR_INVALID case, each reached by mending the one before it; MRT_ERR_NO_SCENE and MRT_ERR_PENDING after them; count == 0
    writes nothing."""
    L = capi.load()
    w, h = 64, 48
    n = w * h
    ctx = capi.Context(0)
    dev = Dev(ctx)
    verts, layers, cam_def, shade = emitter_scene("room")
    try:
        cam = capi.camera_look(cam_def[0], cam_def[1], w, h, cam_def[2])
        d_rays, d_hits, d_rows, d_out = dev.alloc(n * 32), dev.alloc(n * 32), dev.alloc(n * 64), dev.alloc(n * 16)
        d_mask, d_em = dev.put(np.full(n, 7, np.uint8)), dev.put(np.full(n, 0x5A5A5A5A, np.uint32))   # (7 is an emitter: a word no table gives)

        def call(grid, a):
            desc = None if a["desc"] is None else C.byref(capi.EmitterSelect(a["frame"], 512, None, a["out_emitter"]))
            if grid:
                return L.mrt_cast_grid_emitter_shadows(ctx.h, C.byref(cam), w, h, 0, h, a["hits"], desc, a["mask"], 0xFFFFFFFF, a["flags"])
            return L.mrt_cast_emitter_shadows(ctx.h, a["rays"], a["hits"], a["count"], desc, a["mask"], 0xFFFFFFFF, a["flags"])

        for grid in (False, True):
            # everything wrong at once; mended in the header's order, the call stays invalid until the last is mended
            a = dict(rays=None, hits=None, desc=None, mask=None, out_emitter=None, flags=capi.FLAG_COHERENT, frame=T.PATH_MAX_FRAME + 1, count=n)
            mend = [("rays", d_rays), ("hits", d_hits), ("desc", True), ("mask", d_mask), ("out_emitter", d_em), ("flags", capi.FLAG_ASYNC),
                    ("frame", T.PATH_MAX_FRAME)]
            seen = []
            for step, (k, v) in enumerate(mend):
                assert call(grid, a) == capi.ERR_INVALID, (grid, step, k)
                seen.append(ctx.L.mrt_last_error(ctx.h).decode())
                a[k] = v
            want = ["rays", "hits", "descriptor", "mask", "d_out_emitter", "flag", "frame"]
            assert all(x in y for x, y in zip(want[grid:], seen[grid:])), seen           # (the grid form has no rays argument)
            assert call(grid, a) == capi.ERR_NO_SCENE, grid                             # valid, and no scene yet
            ctx.synchronize()
        assert call(True, dict(a, flags=capi.FLAG_HOST_LAYOUT)) == capi.ERR_INVALID      # grid records are mrt_hit32
        nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts))
        ctx.upload_scene(capi.make_triangles(verts, layers=layers), nodes, prim_idx)
        ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids)
        assert ctx.build_emitters(world_tris(verts, layers))[0] > 0
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        ctx.generate_grid(cam, w, h, 0, h, d_rays)
        ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows)
        a["flags"] = 0
        # no records: MRT_OK, nothing written
        assert call(False, dict(a, count=0)) == capi.MRT_OK
        assert L.mrt_cast_grid_emitter_shadows(ctx.h, C.byref(cam), w, h, 9, 9, d_hits, C.byref(capi.EmitterSelect(0, 512, None, d_em)), d_mask,
                                               0xFFFFFFFF, 0) == capi.MRT_OK
        assert (dev.get(d_mask, n, np.uint8) == 7).all() and (dev.get(d_em, n, np.uint32) == 0x5A5A5A5A).all()
        # the build: its pointer, its flag
        assert L.mrt_build_emitters(ctx.h, None, 5, 0) == capi.ERR_INVALID and L.mrt_build_emitters(ctx.h, d_rays, 5, capi.BUILD_SAFE_HANDOFF) == capi.ERR_INVALID
        assert L.mrt_build_emitters(ctx.h, None, 5, 2) == capi.ERR_INVALID and "tris" in ctx.L.mrt_last_error(ctx.h).decode()
        # a dispatch pending: after the invalid cases, before any work
        ctx.submit(po.grid_rays(cam_def[0], cam_def[1], w, h, cam_def[2]))
        assert call(False, dict(a, frame=T.PATH_MAX_FRAME + 1)) == capi.ERR_INVALID
        assert call(False, a) == capi.ERR_PENDING and call(True, a) == capi.ERR_PENDING
        assert L.mrt_build_emitters(ctx.h, d_rays, 5, capi.BUILD_TRIS_ON_DEVICE) == capi.ERR_PENDING and L.mrt_clear_emitters(ctx.h) == capi.ERR_PENDING
        ctx.collect()
        assert call(False, a) == capi.MRT_OK and call(True, a) == capi.MRT_OK
        assert (dev.get(d_em, n, np.uint32) != 0x5A5A5A5A).all()

        # the light call
        def lcall(grid, l):
            desc = None if l["desc"] is None else C.byref(capi.EmitterSelect(l["frame"], 512, None, l["em"]))
            out = None if l["out"] is None else C.byref(capi.LightOut(l["rgba"]))
            if grid:
                return L.mrt_light_grid_emitter_surfaces(ctx.h, C.byref(cam), w, h, 0, h, l["hits"], l["rows"], desc, None, l["acc"], out, l["flags"])
            return L.mrt_light_emitter_surfaces(ctx.h, l["rays"], l["hits"], l["rows"], l["count"], desc, None, l["acc"], out, l["flags"])

        for grid in (False, True):
            l = dict(rays=None, hits=None, rows=None, desc=None, em=None, out=None, rgba=None, flags=capi.FLAG_BOOL_OUT, acc=2, frame=T.PATH_MAX_FRAME + 1, count=n)
            mend = [("rays", d_rays), ("hits", d_hits), ("rows", d_rows), ("desc", True), ("em", d_em), ("out", True), ("rgba", d_out), ("flags", 0),
                    ("acc", 1), ("frame", 0)]
            seen = []
            for step, (k, v) in enumerate(mend):
                assert lcall(grid, l) == capi.ERR_INVALID, (grid, step, k)
                seen.append(ctx.L.mrt_last_error(ctx.h).decode())
                l[k] = v
            want = ["rays", "hits", "rows", "descriptor", "d_out_emitter", "output", "output", "flag", "accumulate", "frame"]
            assert all(x in y for x, y in zip(want[grid:], seen[grid:])), seen
            assert lcall(grid, l) == capi.MRT_OK
        assert lcall(True, dict(l, flags=capi.FLAG_HOST_LAYOUT)) == capi.ERR_INVALID
        ctx.h2d(d_out, np.full(n * 4, 3.0, F))
        assert lcall(False, dict(l, count=0)) == capi.MRT_OK and (dev.get(d_out, n * 4, F) == 3).all()
        # the step: mrt_path_step's refusals, then the lobe bytes
        env = np.ascontiguousarray(environment(), dtype=T.ENVIRONMENT).reshape(1)
        d_state, d_sel, d_lobe = dev.alloc(n * 32), dev.alloc(n), dev.put(np.full(n, 2, np.uint8))
        ctx.path_init(d_state, n)

        def scall(grid, bounce, lobe, max_bounces=3, flags=0):
            desc = capi.PathStepDesc(0, bounce, max_bounces, 0, d_out, d_state, env.ctypes.data, d_sel, None, None)
            if grid:
                return L.mrt_path_grid_step_emitters(ctx.h, C.byref(cam), w, h, 0, h, d_hits, d_rows, C.byref(desc), lobe, flags)
            return L.mrt_path_step_emitters(ctx.h, d_rays, d_hits, d_rows, n, C.byref(desc), lobe, flags)

        for grid in (False, True):
            assert scall(grid, 4, None) == capi.ERR_INVALID and "max_bounces" in ctx.L.mrt_last_error(ctx.h).decode()
            assert scall(grid, 1, None, flags=capi.FLAG_COHERENT) == capi.ERR_INVALID and "flag" in ctx.L.mrt_last_error(ctx.h).decode()
            assert scall(grid, 1, None) == capi.ERR_INVALID and "d_prev_lobe" in ctx.L.mrt_last_error(ctx.h).decode()
            assert scall(grid, 0, None) == capi.MRT_OK and scall(grid, 1, d_lobe) == capi.MRT_OK
        assert scall(True, 0, None, flags=capi.FLAG_HOST_LAYOUT) == capi.ERR_INVALID
    finally:
        dev.free()
        ctx.close()


def test_async_on_a_callers_stream_then_a_dependent_read(built):
    """The cast, the light call and the step ASYNC on a stream of the caller's, a copy of their outputs queued behind them on that stream
    and one wait for it: what the blocking calls on the context's own stream gave."""
    lit = Lit("room", *GRID, T.path_emitter_draw(1))
    ctx, dev, n = lit.wd.ctx, lit.wd.dev, lit.n
    cs = Caller()
    try:
        env = environment()
        outs = []
        for flags in (0, capi.FLAG_ASYNC):
            d_mask, d_em, d_rgba = dev.put(np.full(n, 9, np.uint8)), dev.put(np.full(n, 9, np.uint32)), dev.put(np.zeros(n * 4, F))
            d_state, d_sel = dev.alloc(n * 32), dev.put(np.full(n, 9, np.uint8))
            d_res = dev.put(np.zeros(n * 54, np.uint8))
            ctx.path_init(d_state, n)
            if flags:
                ctx.set_stream(cs.s)
            ctx.cast_grid_emitter_shadows(lit.cam, lit.w, lit.h, lit.d_shits, d_mask, d_em, FRAME, lit.draw, flags=flags)
            ctx.light_grid_emitter_surfaces(lit.cam, lit.w, lit.h, lit.d_shits, lit.d_rows, d_em, d_rgba, d_mask, FRAME, lit.draw, flags=flags)
            ctx.path_grid_step_emitters(lit.cam, lit.w, lit.h, lit.d_shits, lit.d_rows, d_rgba, d_state, env, d_sel, None, FRAME, 0, 3, flags=flags)
            if flags:
                cs.copy(d_res, d_mask, n)
                cs.copy(d_res + n, d_em, n * 4)
                cs.copy(d_res + 5 * n, d_rgba, n * 16)
                cs.copy(d_res + 21 * n, d_state, n * 32)
                cs.copy(d_res + 53 * n, d_sel, n)
                cs.sync()
                ctx.set_stream(0)
                outs.append(dev.get(d_res, n * 54, np.uint8))
            else:
                outs.append(np.concatenate([dev.get(d_mask, n, np.uint8), dev.get(d_em, n * 4, np.uint8), dev.get(d_rgba, n * 16, np.uint8),
                                            dev.get(d_state, n * 32, np.uint8), dev.get(d_sel, n, np.uint8)]))
        np.testing.assert_array_equal(outs[1], outs[0])
        assert (outs[0][:n] == 0).any() and (outs[0][53 * n:] == 1).any()
    finally:
        ctx.set_stream(0)
        lit.close()
        cs.destroy()
