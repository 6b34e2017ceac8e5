"""mrt_cast_selected_shadows / mrt_cast_grid_selected_shadows and mrt_light_selected_surfaces / mrt_light_grid_selected_surfaces: one
light per record, drawn from the pixel's own stream, one shadow ray to it and that light's term scaled by the number of lights.  The
light bytes are held to nee.select_lights and the lit bytes to the oracle's any-hit answer for nee.selected_shadow_rays, byte for byte;
every lit byte is also the byte mrt_cast_shadows writes for the same (record, light) pair; the light call is held to
nee.selected_direct as uint32 words.  Flat and two-level synth.room() and a soup; the light list of test_shadow_gpu.py cut to 1, 3 and 5
lights and grown to 16; a grid with whole and clipped tiles, a row band of it, the array form in both layouts and one array batch of
77 000 records (the count at which test_shadow_gpu.py's grids reach the persistent kernels).  A whole frame of the queue INTEGRATION §4
gives, against the same loop in numpy.  Refusals in the header's order; ASYNC on a caller's stream."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import capi, nee, types as T
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import path as P
from oracle import pyoracle as po
from test_caller_stream_gpu import Caller
from test_hemisphere_gpu import DEV, Dev, Run, hit_point, scene
from test_lighting_gpu import Lit, environment
from test_shadow_gpu import light, lights_for
from test_surface_gpu import words

pytestmark = pytest.mark.gpu

F = np.float32
FAR = F(1e30)
FRAME = 5
GRID = (100, 37)            # 12 whole tiles and a clipped column and row of them; 3 700 records: the plain kernels
BAND = (5, 29)
BATCH = (200, 385)          # 77 000 records as an array: the persistent kernels
PLAIN = {"room": "trace_selected_shadow_lane_kernel<", "room_tl": "trace_selected_shadow_two_level_kernel<", "soup": "trace_selected_shadow_lane_kernel<"}


def cut(sc, org_of_a_hit, n_lights):
    """test_shadow_gpu.py's list (directional, point, spot, one with cast_shadows = 0, a point light on one record's shadow origin) cut
    to its first n lights, or grown to 16 by repeating its lights at new positions and directions."""
    base = lights_for(sc, org_of_a_hit)
    if n_lights <= len(base):
        return base[:n_lights].copy()
    rng = np.random.default_rng(2700 + n_lights)
    more = base[np.arange(n_lights - len(base)) % 4].copy()
    more["position"] += rng.uniform(-1.5, 1.5, more["position"].shape).astype(F)
    more["direction"] += rng.uniform(-0.3, 0.3, more["direction"].shape).astype(F)
    return np.concatenate([base, more])


def check_selected(sc, dev, light_bytes, mask, all_mask, pixel, draw, lights, pos, nrm, hit, select=None, query_mask=0xFFFFFFFF, what=""):
    """The three checks of one cast: the light bytes against nee.select_lights, the lit bytes against the oracle, and both against the
    all-lights mask of mrt_cast_shadows without numpy's rays."""
    n = hit.shape[0]
    want_light = nee.select_lights(pixel, FRAME, draw, len(lights), hit, select)
    np.testing.assert_array_equal(light_bytes, want_light, err_msg=what + ": d_out_light")
    rays, traced = nee.selected_shadow_rays(pos, nrm, hit, lights, want_light)
    np.testing.assert_array_equal(mask, sc.lit(rays, traced, query_mask), err_msg=what + ": d_mask against the oracle")
    on = light_bytes != T.LIGHT_NONE
    assert (mask[~on] == 1).all(), what
    at = light_bytes[on].astype(np.int64) * n + np.flatnonzero(on)
    np.testing.assert_array_equal(mask[on], all_mask[at], err_msg=what + ": d_mask against mrt_cast_shadows' byte of the pair")
    return want_light


def grid_form(kind, n_lights, y0, y1, draw):
    w, h = GRID
    run = Run(kind, w, h, y0, y1)
    ctx, dev, n, sc = run.ctx, run.dev, run.n, run.sc
    try:
        hit = run.hits["prim_id"] != -1
        pos = hit_point(run.rays, run.hits)
        first = int(np.flatnonzero(hit)[0])
        lights = cut(sc, pos[first] + run.hits["normal"][first] * F(1e-3), n_lights)
        d_all, d_mask, d_light = dev.alloc(n * n_lights), dev.put(np.full(n + 64, 0x5A, np.uint8)), dev.put(np.full(n + 64, 0x5A, np.uint8))
        ctx.cast_grid_shadows(run.cam, w, h, run.d_hits, lights, d_all, y0=y0, y1=run.y1)
        all_mask = dev.get(d_all, n * n_lights, np.uint8)
        ctx.cast_grid_selected_shadows(run.cam, w, h, run.d_hits, lights, d_mask, d_light, FRAME, draw, y0=y0, y1=run.y1)
        assert ctx.last_kernel_variant().startswith(PLAIN[kind]), ctx.last_kernel_variant()
        mask, lb = dev.get(d_mask, n + 64, np.uint8), dev.get(d_light, n + 64, np.uint8)
        assert (mask[n:] == 0x5A).all() and (lb[n:] == 0x5A).all()                       # nothing behind the last record
        pixel = np.arange(n, dtype=np.uint64) + y0 * w                                   # the whole grid's index
        got = check_selected(sc, dev, lb[:n], mask[:n], all_mask, pixel, draw, lights, pos, run.hits["normal"], hit, what="grid")
        if n_lights >= 3:
            assert len(np.unique(got[hit])) == n_lights and (kind == "soup" or (mask[:n] == 0).any())
        return got, mask[:n]
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["room", "room_tl", "soup"])
@pytest.mark.parametrize("n_lights", [1, 3, 5, 16])
def test_grid_and_band_against_the_oracle(built, kind, n_lights):
    """Grid 100 x 37 whole, and its rows [5, 29): the band selects, and shadows, what the whole frame does."""
    draw = T.path_select_draw(1)
    whole = grid_form(kind, n_lights, 0, GRID[1], draw)
    band = grid_form(kind, n_lights, BAND[0], BAND[1], draw)
    a, b = BAND[0] * GRID[0], BAND[1] * GRID[0]
    np.testing.assert_array_equal(whole[0][a:b], band[0])
    if n_lights < 5:   # (the fifth light sits on the first hit of the cast it was made for: the band's list differs from the frame's there)
        np.testing.assert_array_equal(whole[1][a:b], band[1])


def array_forms(kind, n_lights, w, h, draw, persistent):
    sc = scene(kind)
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        n = w * h
        rays = po.grid_rays(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
        d_rays, d_h32 = dev.put(rays), dev.alloc(n * 32)
        ctx.cast(d_rays, d_h32, count=n, flags=DEV)
        hits = dev.get(d_h32, n, T.HIT32)
        hit = hits["prim_id"] != -1
        pos = hit_point(rays, hits)
        first = int(np.flatnonzero(hit)[0])
        lights = cut(sc, pos[first] + hits["normal"][first] * F(1e-3), n_lights)
        pixel = np.arange(n, dtype=np.uint64)                                            # the array form: the record's index
        d_all, d_mask, d_light = dev.alloc(n * n_lights), dev.alloc(n), dev.alloc(n)
        ctx.cast_shadows(d_rays, d_h32, n, lights, d_all)
        all_mask = dev.get(d_all, n * n_lights, np.uint8)
        ctx.cast_selected_shadows(d_rays, d_h32, n, lights, d_mask, d_light, FRAME, draw)
        v = ctx.last_kernel_variant()
        assert ("selected_shadow_persistent" in v) if persistent else v.startswith(PLAIN[kind]), v
        check_selected(sc, dev, dev.get(d_light, n, np.uint8), dev.get(d_mask, n, np.uint8), all_mask, pixel, draw, lights, pos,
                       hits["normal"], hit, what="ray32")
        if persistent:
            return
        # the reference's host layout: the record carries the position
        hrays = po.make_host_rays(rays)
        d_hr, d_h44 = dev.put(hrays), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        h44 = dev.get(d_h44, n, T.HOST_HIT44)
        d_mask44, d_light44 = dev.alloc(n), dev.alloc(n)
        ctx.cast_shadows(d_hr, d_h44, n, lights, d_all, flags=capi.FLAG_HOST_LAYOUT)
        all44 = dev.get(d_all, n * n_lights, np.uint8)
        ctx.cast_selected_shadows(d_hr, d_h44, n, lights, d_mask44, d_light44, FRAME, draw, flags=capi.FLAG_HOST_LAYOUT)
        assert ctx.last_kernel_variant().startswith(PLAIN[kind]), ctx.last_kernel_variant()
        check_selected(sc, dev, dev.get(d_light44, n, np.uint8), dev.get(d_mask44, n, np.uint8), all44, pixel, draw, lights, h44["position"],
                       h44["normal"], h44["prim_id"] != T.NO_HIT, what="host layout")
    finally:
        dev.free()
        ctx.close()


@pytest.mark.parametrize("kind", ["room", "room_tl", "soup"])
@pytest.mark.parametrize("n_lights", [1, 3, 5, 16])
def test_array_forms_against_the_oracle(built, kind, n_lights):
    array_forms(kind, n_lights, GRID[0], GRID[1], T.path_select_draw(0), False)


@pytest.mark.parametrize("kind", ["room", "room_tl", "soup"])
@pytest.mark.parametrize("n_lights", [1, 3, 5, 16])
def test_a_large_batch_runs_the_persistent_kernels(built, kind, n_lights):
    array_forms(kind, n_lights, BATCH[0], BATCH[1], T.path_select_draw(2), True)


@pytest.mark.parametrize("kind", ["soup", "room"])
def test_select_bytes_misses_and_query_mask(built, kind):
    """A d_select with zeros and (the soup) misses among the records: MRT_LIGHT_NONE, lit.  A query_mask that hides the occluders (the
    room's walls): the selection is the same and the lit bytes are the oracle's under that mask."""
    w, h = GRID
    run = Run(kind, w, h)
    ctx, dev, n, sc = run.ctx, run.dev, run.n, run.sc
    try:
        hit = run.hits["prim_id"] != -1
        assert kind != "soup" or (~hit).any()
        pos = hit_point(run.rays, run.hits)
        first = int(np.flatnonzero(hit)[0])
        lights = cut(sc, pos[first] + run.hits["normal"][first] * F(1e-3), 5)
        select = (np.arange(n) % 3 != 1).astype(np.uint8)
        pixel = np.arange(n, dtype=np.uint64)
        draw = T.path_select_draw(3)
        d_sel, d_all, d_mask, d_light = dev.put(select), dev.alloc(5 * n), dev.alloc(n), dev.alloc(n)
        for qm in (0xFFFFFFFF, 1):
            ctx.cast_grid_shadows(run.cam, w, h, run.d_hits, lights, d_all, query_mask=qm)
            all_mask = dev.get(d_all, 5 * n, np.uint8)
            ctx.cast_grid_selected_shadows(run.cam, w, h, run.d_hits, lights, d_mask, d_light, FRAME, draw, d_select=d_sel, query_mask=qm)
            lb, mask = dev.get(d_light, n, np.uint8), dev.get(d_mask, n, np.uint8)
            check_selected(sc, dev, lb, mask, all_mask, pixel, draw, lights, pos, run.hits["normal"], hit, select, qm, what=f"query_mask {qm}")
            assert (lb[select == 0] == T.LIGHT_NONE).all() and (lb[~hit] == T.LIGHT_NONE).all() and (lb[hit & (select != 0)] < 5).all()
            if qm == 1:
                assert kind == "soup" or (mask != full).any()                            # the walls no longer shadow
            full = mask
    finally:
        run.close()


@pytest.mark.parametrize("kind", ["soup", "room_tl"])
def test_one_light_is_the_all_lights_pair(built, kind):
    """n_lights == 1: the mask is mrt_cast_shadows' mask byte for byte and mrt_light_selected_surfaces is mrt_light_surfaces word for
    word, with and without the environment -- for a light of each kind and one that casts no shadows."""
    lit = Lit(kind, *GRID)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        d_m1, d_ms, d_light, d_a, d_b = dev.alloc(n), dev.alloc(n), dev.alloc(n), dev.alloc(n * 16), dev.alloc(n * 16)
        for l in (0, 1, 2, 4):
            one = lit.lights[l:l + 1]
            ctx.cast_grid_shadows(run.cam, run.w, run.h, run.d_hits, capi.shadow_lights(one), d_m1)
            ctx.cast_grid_selected_shadows(run.cam, run.w, run.h, run.d_hits, capi.shadow_lights(one), d_ms, d_light, FRAME, T.path_select_draw(0))
            np.testing.assert_array_equal(dev.get(d_ms, n, np.uint8), dev.get(d_m1, n, np.uint8))
            lb = dev.get(d_light, n, np.uint8)
            assert (lb[lit.hit] == 0).all() and (lb[~lit.hit] == T.LIGHT_NONE).all()
            for env in (None, lit.env):
                for m in (d_m1, None):
                    ctx.light_grid_surfaces(run.cam, run.w, run.h, run.d_hits, lit.d_rows, one, d_a, m, env)
                    ctx.light_grid_selected_surfaces(run.cam, run.w, run.h, run.d_hits, lit.d_rows, one, d_light, d_b, m, env)
                    a, b = dev.get(d_a, n * 4, np.uint32), dev.get(d_b, n * 4, np.uint32)
                    np.testing.assert_array_equal(b, a, err_msg=f"light {l}")
            assert (dev.get(d_a, n * 4, F).reshape(-1, 4)[lit.hit, :3] > 0).any()
    finally:
        lit.close()


@pytest.mark.parametrize("kind", ["room", "soup"])
@pytest.mark.parametrize("n_lights", [5, 16])
def test_light_call_matches_the_restatement(built, kind, n_lights):
    """Rows resolved from the scene: the grid form, the array form and the host-layout array form against nee.selected_direct, with the
    bytes the selected cast wrote; with and without the mask and the environment."""
    lit = Lit(kind, *GRID)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        lights = lit.lights[:n_lights]
        shadow = capi.shadow_lights(lights)
        d_mask, d_light, d_out = dev.alloc(n), dev.alloc(n), dev.put(np.full(n * 4 + 64, -7.5, F))
        ctx.cast_grid_selected_shadows(run.cam, run.w, run.h, run.d_hits, shadow, d_mask, d_light, FRAME, T.path_select_draw(0))
        mask, lb = dev.get(d_mask, n, np.uint8), dev.get(d_light, n, np.uint8)
        assert (mask == 0).any() and len(np.unique(lb[lit.hit])) == n_lights
        d = run.rays["direction"]
        d_rays = dev.put(run.rays)
        for env in (lit.env, None):
            for m, dm in ((mask, d_mask), (None, None)):
                want = nee.selected_direct(lit.rows, lit.p, d, lights, lb, m, env, lit.hit)
                ctx.light_grid_selected_surfaces(run.cam, run.w, run.h, run.d_hits, lit.d_rows, lights, d_light, d_out, dm, env)
                got = dev.get(d_out, n * 4 + 64, F)
                np.testing.assert_array_equal(words(got[:n * 4].reshape(-1, 4)), words(want), err_msg="grid form")
                assert (got[n * 4:] == F(-7.5)).all()
                ctx.light_selected_surfaces(d_rays, run.d_hits, lit.d_rows, n, lights, d_light, d_out, dm, env)
                np.testing.assert_array_equal(words(dev.get(d_out, n * 4, F).reshape(-1, 4)), words(want), err_msg="array form")
        assert np.isfinite(want).all() and (want[lit.hit, :3] > 0).any()
        # the reference's host layout
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44, d_rows44 = dev.put(hrays), dev.alloc(n * 44), dev.alloc(n * 64)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        ctx.resolve_surfaces(d_hr, d_h44, n, d_rows44, flags=capi.FLAG_HOST_LAYOUT)
        ctx.cast_selected_shadows(d_hr, d_h44, n, shadow, d_mask, d_light, FRAME, T.path_select_draw(0), flags=capi.FLAG_HOST_LAYOUT)
        h44, rows44 = dev.get(d_h44, n, T.HOST_HIT44), dev.get(d_rows44, n, T.SURFACE64)
        mask, lb = dev.get(d_mask, n, np.uint8), dev.get(d_light, n, np.uint8)
        want = nee.selected_direct(rows44, h44["position"], hrays["direction"], lights, lb, mask, lit.env, h44["prim_id"] != T.NO_HIT)
        ctx.light_selected_surfaces(d_hr, d_h44, d_rows44, n, lights, d_light, d_out, d_mask, lit.env, flags=capi.FLAG_HOST_LAYOUT)
        np.testing.assert_array_equal(words(dev.get(d_out, n * 4, F).reshape(-1, 4)), words(want), err_msg="host layout")
    finally:
        lit.close()


def test_light_call_on_hand_made_rows(built):
    """Rows, records and rays made by hand, so that every skip occurs and is counted: a light byte of 0xFF, one past the list, a mask
    byte of 0, a point light out of range, a surface facing away, a spot light seen from outside its cone."""
    from test_selected_nee_cpu import five_lights, hand_made
    rows, p0, d = hand_made(side=19)                                                    # 361 records: two workgroups, the last ragged
    n = rows.shape[0]
    rays = np.zeros(n, T.RAY32)
    rays["direction"], rays["origin"], rays["t_max"] = d, p0 - d * F(5), FAR
    hits = np.zeros(n, T.HIT32)
    hits["t"], hits["prim_id"], hits["normal"] = 5, np.arange(n), rows["normal"]
    hits["prim_id"][7::31] = -1
    hit = hits["prim_id"] != -1
    p = hit_point(rays, hits)                                                            # o + d * t, as the kernel makes it
    ls = five_lights()
    rows["normal"][3::17] = -rows["normal"][3::17]                                       # facing away from everything above
    rng = np.random.default_rng(12)
    lb = rng.integers(0, 5, n).astype(np.uint8)
    lb[::13], lb[5::29] = T.LIGHT_NONE, 5
    lb[~hit] = T.LIGHT_NONE
    mask = (np.arange(n) % 6 != 2).astype(np.uint8)
    # every case occurs (float64 geometry: this only counts)
    v = Lg.view_dir(d)
    seen = dict(none=bool(((lb == T.LIGHT_NONE) & hit).any()), past=bool(((lb == 5) & hit).any()), masked=False, beyond=False, away=False, outside=False)
    for k in range(5):
        mine = hit & (lb == k)
        _, active, _, atten = Lg.light_term(rows, p, v, ls[k])
        seen["masked"] |= bool((mine & active & (mask == 0)).any())
        if ls[k]["type"] != T.LIGHT_DIRECTIONAL:
            dist = np.linalg.norm(ls[k]["position"].astype(np.float64) - p, axis=1)
            seen["beyond"] |= bool((mine & (dist > ls[k]["range"])).any())
            L = (ls[k]["position"].astype(np.float64) - p) / dist[:, None]
            inside = dist <= ls[k]["range"]
            if ls[k]["type"] == T.LIGHT_SPOT:
                out = inside & (L @ ls[k]["direction"].astype(np.float64) < np.cos(np.float64(ls[k]["spot_angle"])) - 1e-4)
                seen["outside"] |= bool((mine & out).any())
                inside &= ~out
            seen["away"] |= bool((mine & inside & ((rows["normal"] * L).sum(axis=1) < -1e-3)).any())
    assert all(seen.values()), seen
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        d_rays, d_hits, d_rows, d_lb, d_mask = dev.put(rays), dev.put(hits), dev.put(rows), dev.put(lb), dev.put(mask)
        d_out = dev.put(np.full(n * 4 + 64, -7.5, F))
        for env in (None, environment()):
            for m, dm in ((mask, d_mask), (None, None)):
                want = nee.selected_direct(rows, p, d, ls, lb, m, env, hit)
                ctx.light_selected_surfaces(d_rays, d_hits, d_rows, n, ls, d_lb, d_out, dm, env)
                got = dev.get(d_out, n * 4 + 64, F)
                np.testing.assert_array_equal(words(got[:n * 4].reshape(-1, 4)), words(want))
                assert (got[n * 4:] == F(-7.5)).all()
        bare = nee.selected_direct(rows, p, d, ls, lb, mask, None, hit)               # (checked above: the first of the four)
        assert (bare[hit & ((lb >= 5) | (mask == 0)), :3] == 0).all() and (bare[hit, :3] > 0).any() and (bare[~hit] == 0).all()
    finally:
        dev.free()
        ctx.close()


def test_whole_frame_against_the_numpy_loop(built):
    """Grid 64 x 48, max_bounces = 3, 5 lights: per bounce cast -> resolve -> selected shadows with select_draw =
    MRT_PATH_SELECT_DRAW(bounce) -> selected light with env = NULL -> step -> bounce cast, every call ASYNC; the final state word for
    word against path.path_step fed by nee.selected_direct on the device's records."""
    w, h, bounces, n_lights = 64, 48, 3, 5
    lit = Lit("soup", w, h)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    A = capi.FLAG_ASYNC
    try:
        lights, env = lit.lights[:n_lights], lit.env
        shadow = capi.shadow_lights(lights)
        pairs = [(dev.alloc(n * 32), dev.alloc(n * 32)), (dev.alloc(n * 32), dev.alloc(n * 32))]
        d_rows, d_pairs, d_shits, d_mask, d_light, d_direct = dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 32), dev.alloc(n), dev.alloc(n), dev.alloc(n * 16)
        d_state, d_select = dev.alloc(n * 32), dev.alloc(n)
        d_counts = dev.put(np.zeros(bounces + 1, np.uint32))
        ctx.path_init(d_state, n, flags=A)
        state = P.init_state(n)
        pixel = np.arange(n, dtype=np.uint64)
        rays_host = run.rays
        used = np.zeros(n_lights, np.int64)
        for b in range(bounces + 1):
            cur_rays, cur_hits = (None, run.d_hits) if b == 0 else pairs[b & 1]
            nxt_rays, nxt_hits = pairs[(b + 1) & 1]
            draw = T.path_select_draw(b)
            kw = dict(frame=FRAME, bounce=b, max_bounces=bounces, d_active_count=d_counts + 4 * b, flags=A)
            if b == 0:
                ctx.resolve_grid_surfaces(run.cam, w, h, cur_hits, d_rows, d_pairs, d_shits, flags=A)
                ctx.cast_grid_selected_shadows(run.cam, w, h, cur_hits, shadow, d_mask, d_light, FRAME, draw, flags=A)
                ctx.light_grid_selected_surfaces(run.cam, w, h, cur_hits, d_rows, lights, d_light, d_direct, d_mask, None, flags=A)
                ctx.path_grid_step(run.cam, w, h, d_shits, d_rows, d_direct, d_state, env, d_select, **kw)
            else:
                ctx.resolve_surfaces(cur_rays, cur_hits, n, d_rows, d_pairs, d_shits, flags=A)
                ctx.cast_selected_shadows(cur_rays, cur_hits, n, shadow, d_mask, d_light, FRAME, draw, d_select=d_select, flags=A)
                ctx.light_selected_surfaces(cur_rays, cur_hits, d_rows, n, lights, d_light, d_direct, d_mask, None, flags=A)
                ctx.path_step(cur_rays, d_shits, d_rows, n, d_direct, d_state, env, d_select, **kw)
            if b < bounces:
                bk = dict(frame=FRAME, first_draw=P.first_draw(b), t_max=FAR, d_select=d_select, d_surface=d_pairs, d_out_rays=nxt_rays, flags=A)
                if b == 0:
                    ctx.cast_grid_bounce(run.cam, w, h, d_shits, nxt_hits, **bk)
                else:
                    ctx.cast_bounce(cur_rays, d_shits, n, nxt_hits, **bk)
            ctx.synchronize()
            # the same bounce in numpy, on the device's records
            hits, shits = dev.get(cur_hits, n, T.HIT32), dev.get(d_shits, n, T.HIT32)
            rows, mask = dev.get(d_rows, n, T.SURFACE64), dev.get(d_mask, n, np.uint8)
            hit = hits["prim_id"] != -1
            prev = None if b == 0 else select
            lb = nee.select_lights(pixel, FRAME, draw, n_lights, hit, prev)
            np.testing.assert_array_equal(dev.get(d_light, n, np.uint8), lb, err_msg=f"light bytes of bounce {b}")
            used += np.bincount(lb[lb != T.LIGHT_NONE], minlength=n_lights)
            direct = nee.selected_direct(rows, hit_point(rays_host, hits), rays_host["direction"], lights, lb, mask, None, hit)
            np.testing.assert_array_equal(words(dev.get(d_direct, n * 4, F).reshape(-1, 4)), words(direct), err_msg=f"direct of bounce {b}")
            state, select, _, count = P.path_step(state, rows, hit, shits["normal"], rays_host["direction"], direct, env, pixel, FRAME, b, bounces)
            np.testing.assert_array_equal(words(dev.get(d_state, n, T.PATH_STATE)).reshape(-1, 8), words(state).reshape(-1, 8), err_msg=f"state after bounce {b}")
            np.testing.assert_array_equal(dev.get(d_select, n, np.uint8), select)
            assert int(dev.get(d_counts + 4 * b, 1, np.uint32)[0]) == count
            if b < bounces:
                rays_host = dev.get(nxt_rays, n, T.RAY32)
            if count == 0:
                break
        assert b >= 2 and (used > 0).all()                                            # (the loop ends early only when nothing is active)
        assert (state["active"] == 0).all() and (state["radiance"] > 0).any() and np.isfinite(state["radiance"]).all()
    finally:
        lit.close()


def test_refusals_in_the_stated_order_and_empty_calls(built):
    """Every MRT_ERR_INVALID case, each reached by mending the one before it; MRT_ERR_NO_SCENE and MRT_ERR_PENDING after them;
    n_lights == 0 and count == 0 write nothing."""
    L = capi.load()
    sc = scene("room")
    w, h = 64, 48
    n = w * h
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        lights = np.concatenate([light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5)), light(T.LIGHT_DIRECTIONAL, direction=(0.3, 1.0, 0.2))])
        many = np.concatenate([lights] * 9)
        bad_type = lights.copy()
        bad_type["type"][1] = 3
        cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
        d_rays, d_hits = dev.alloc(n * 32), dev.alloc(n * 32)
        d_mask, d_light = dev.put(np.full(n, 7, np.uint8)), dev.put(np.full(n, 7, np.uint8))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)

        def call(grid, a):
            desc = None if a["desc"] is None else C.byref(capi.LightSelect(a["frame"], 256, None, a["out_light"]))
            if grid:
                return L.mrt_cast_grid_selected_shadows(ctx.h, C.byref(cam), w, h, 0, h, a["hits"], desc, a["lights"], a["n"], a["mask"], 0xFFFFFFFF, a["flags"])
            return L.mrt_cast_selected_shadows(ctx.h, a["rays"], a["hits"], a["count"], desc, a["lights"], a["n"], a["mask"], 0xFFFFFFFF, a["flags"])

        for grid in (False, True):
            # everything wrong at once; mended in the header's order, the call stays invalid until the last is mended
            a = dict(rays=None, hits=None, desc=None, mask=None, out_light=None, lights=None, n=17, flags=capi.FLAG_COHERENT,
                     frame=T.PATH_MAX_FRAME + 1, count=n)
            mend = [("rays", d_rays), ("hits", d_hits), ("desc", True), ("mask", d_mask), ("out_light", d_light), ("lights", ptr(many)),
                    ("flags", capi.FLAG_ASYNC), ("n", 2), ("lights", ptr(lights)), ("frame", T.PATH_MAX_FRAME)]
            for step, (k, v) in enumerate(mend):
                assert call(grid, a) == capi.ERR_INVALID, (grid, step, k)
                why = ctx.L.mrt_last_error(ctx.h).decode()
                a[k] = v
                if k == "n":
                    a["lights"] = ptr(bad_type)                                          # now the light type is what is wrong
                    assert "MRT_MAX_LIGHTS" in why, why
                if k == "flags":
                    assert "flag" in why, why
                if k == "frame":
                    assert "frame" in why, why
            assert call(grid, a) == capi.ERR_NO_SCENE, grid                             # valid, and no scene yet
            ctx.synchronize()
        assert call(True, dict(a, flags=capi.FLAG_HOST_LAYOUT)) == capi.ERR_INVALID      # grid records are mrt_hit32
        sc.upload(ctx)
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        ctx.generate_grid(cam, w, h, 0, h, d_rays)
        a["flags"] = 0
        # nothing to select from, or no records: MRT_OK, nothing written
        for grid in (False, True):
            assert call(grid, dict(a, n=0, lights=None)) == capi.MRT_OK
        assert call(False, dict(a, count=0)) == capi.MRT_OK
        assert L.mrt_cast_grid_selected_shadows(ctx.h, C.byref(cam), w, h, 9, 9, d_hits, C.byref(capi.LightSelect(0, 256, None, d_light)), ptr(lights), 2,
                                                d_mask, 0xFFFFFFFF, 0) == capi.MRT_OK
        assert (dev.get(d_mask, n, np.uint8) == 7).all() and (dev.get(d_light, n, np.uint8) == 7).all()
        # a dispatch pending: after the invalid cases, before any work
        ctx.submit(po.grid_rays(sc.cam[0], sc.cam[1], w, h, sc.cam[2]))
        assert call(False, dict(a, frame=T.PATH_MAX_FRAME + 1)) == capi.ERR_INVALID
        assert call(False, a) == capi.ERR_PENDING and call(True, a) == capi.ERR_PENDING
        ctx.collect()
        assert call(False, a) == capi.MRT_OK and call(True, a) == capi.MRT_OK
        assert (dev.get(d_light, n, np.uint8) != 7).all()
        # the light call: d_light is required, the rest as mrt_light_surfaces
        sl = np.zeros(2, T.SHADE_LIGHT)
        sl["range"], sl["type"] = 10, (1, 0)
        d_rows, d_out = dev.alloc(n * 64), dev.alloc(n * 16)
        o = capi.LightOut(d_out)

        def lcall(grid, light_=d_light, flags=0, n_=2, out=o):
            if grid:
                return L.mrt_light_grid_selected_surfaces(ctx.h, C.byref(cam), w, h, 0, h, d_hits, d_rows, ptr(sl), n_, light_, None, None, C.byref(out), flags)
            return L.mrt_light_selected_surfaces(ctx.h, d_rays, d_hits, d_rows, n, ptr(sl), n_, light_, None, None, C.byref(out), flags)

        ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows)
        for grid in (False, True):
            assert lcall(grid) == capi.MRT_OK
            assert lcall(grid, light_=None) == capi.ERR_INVALID
            assert lcall(grid, flags=capi.FLAG_COHERENT) == capi.ERR_INVALID
            assert lcall(grid, n_=17) == capi.ERR_INVALID
            assert lcall(grid, out=capi.LightOut(None)) == capi.ERR_INVALID
        assert lcall(True, flags=capi.FLAG_HOST_LAYOUT) == capi.ERR_INVALID
    finally:
        dev.free()
        ctx.close()


def test_async_on_a_callers_stream_then_a_dependent_read(built):
    """Both calls ASYNC on a stream of the caller's, a copy of their outputs queued behind them on that stream and one wait for it:
    what the blocking calls on the context's own stream gave."""
    lit = Lit("room", *GRID)
    run = lit.run
    ctx, dev, n = run.ctx, run.dev, run.n
    cs = Caller()
    try:
        lights = lit.lights[:5]
        shadow = capi.shadow_lights(lights)
        outs = []
        for flags in (0, capi.FLAG_ASYNC):
            d_mask, d_light, d_rgba = dev.put(np.full(n, 9, np.uint8)), dev.put(np.full(n, 9, np.uint8)), dev.put(np.zeros(n * 4, F))
            d_res = dev.put(np.zeros(n * 18, np.uint8))
            if flags:
                ctx.set_stream(cs.s)
            ctx.cast_grid_selected_shadows(run.cam, run.w, run.h, run.d_hits, shadow, d_mask, d_light, FRAME, T.path_select_draw(1), flags=flags)
            ctx.light_grid_selected_surfaces(run.cam, run.w, run.h, run.d_hits, lit.d_rows, lights, d_light, d_rgba, d_mask, lit.env, flags=flags)
            if flags:
                cs.copy(d_res, d_mask, n)
                cs.copy(d_res + n, d_light, n)
                cs.copy(d_res + 2 * n, d_rgba, n * 16)
                cs.sync()
                ctx.set_stream(0)
                outs.append(dev.get(d_res, n * 18, np.uint8))
            else:
                outs.append(np.concatenate([dev.get(d_mask, n, np.uint8), dev.get(d_light, n, np.uint8), dev.get(d_rgba, n * 16, np.uint8)]))
        np.testing.assert_array_equal(outs[1], outs[0])
        assert (outs[0][:n] == 0).any() and (outs[0][n:2 * n] < 5).any()
    finally:
        ctx.set_stream(0)
        lit.close()
        cs.destroy()
