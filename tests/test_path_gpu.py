"""mrt_path_init / mrt_path_step / mrt_path_grid_step / mrt_path_finish: the path tracer's per-pixel state on the device, held to the
numpy restatement (messyerraytracer_amd/path.py; pinned to the reference by test_path_cpu.py) as uint32 words, byte for byte.  The
scenes, grids and shade data of test_surface_gpu.py, the lights and the environment of test_lighting_gpu.py.  Single steps in the
grid, array and host-layout forms; a band; a whole loop of max_bounces = 4 queued on the device against path.trace_frame fed the
device's own records, in which every case the loop has must occur (the frame number is chosen on the CPU with oracle-traced records
first); agreement with the bounce cast that follows a step; 1, 255, 257 and 2^16 + 1 records with guards; ASYNC; refusals; nothing
resident; primary grids unaffected."""
import ctypes as C

import numpy as np
import pytest

from messyerraytracer_amd import bounce as B
from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import path as P
from oracle import pyoracle as po
from test_hemisphere_gpu import DEV, Dev, hit_point, same, scene, shadow_mask
from test_lighting_gpu import Lit, environment, light_list
from test_surface_gpu import GRIDS, GRID_IDS, KINDS, expected, shade_data, upload, words

pytestmark = pytest.mark.gpu

F = np.float32
FAR = F(1e30)
FRAME = 3
LOOP_KIND, LOOP_GRID, LOOP_LIGHTS, LOOP_BOUNCES = "soup", (96, 72), 4, 4
CASES = ("miss at bounce 0", "miss at a later bounce", "invalid sample", "roulette kill", "roulette survival", "diffuse lobe", "specular lobe",
         "last-bounce stop", "emissive hit", "inactive entry passing through")


class Chain:
    """A Lit (scene, primary grid, rows, shadow mask) with the records that carry the shading normal, the bounce pairs and the direct
    light with env = NULL, on the device and the host: what a bounce-0 step reads."""

    def __init__(self, kind, w, h, y0=0, y1=None, shade=True):
        self.lit = lit = Lit(kind, w, h, y0, y1, shade)
        self.run = run = lit.run
        ctx, dev, n = run.ctx, run.dev, run.n
        self.d_shits, self.d_pairs, self.d_direct = dev.alloc(n * 32), dev.alloc(n * 8), dev.alloc(n * 16)
        ctx.resolve_grid_surfaces(run.cam, run.w, run.h, run.d_hits, d_bounce_surface=self.d_pairs, d_out_hits=self.d_shits, y0=run.y0, y1=run.y1)
        lit.grid(self.d_direct, env=False)
        self.shits, self.direct = dev.get(self.d_shits, n, T.HIT32), dev.get(self.d_direct, n * 4, F).reshape(-1, 4)
        self.env = lit.env
        self.pixel = np.arange(n, dtype=np.uint64) + run.y0 * run.w

    def want(self, state, bounce, max_bounces, frame=FRAME, grid=True, info=None):
        r = self.run
        pixel = self.pixel if grid else np.arange(r.n, dtype=np.uint64)
        return P.path_step(state, self.lit.rows, self.lit.hit, self.shits["normal"], r.rays["direction"], self.direct, self.env, pixel, frame,
                           bounce, max_bounces, info)

    def close(self):
        self.lit.close()


class Outputs:
    """state, select, lobe and count buffers with guard words behind each"""

    def __init__(self, dev, n, state):
        self.dev, self.n = dev, n
        self.d_state = dev.put(np.concatenate([state.view(np.uint32).reshape(-1), np.full(64, 0xA5A5A5A5, np.uint32)]))
        self.d_select, self.d_lobe = dev.put(np.full(n + 64, 0x5A, np.uint8)), dev.put(np.full(n + 64, 0x5A, np.uint8))
        self.d_count = dev.put(np.array([0] + [0xA5A5A5A5] * 15, np.uint32))

    def check(self, want):
        state, select, lobe, count = want
        n, dev = self.n, self.dev
        got = dev.get(self.d_state, n * 8 + 64, np.uint32)
        np.testing.assert_array_equal(got[:n * 8].reshape(-1, 8), state.view(np.uint32).reshape(-1, 8))
        sel, lb, cnt = dev.get(self.d_select, n + 64, np.uint8), dev.get(self.d_lobe, n + 64, np.uint8), dev.get(self.d_count, 16, np.uint32)
        np.testing.assert_array_equal(sel[:n], select)
        np.testing.assert_array_equal(lb[:n], lobe)
        assert cnt[0] == count == int(select.sum())
        assert (got[n * 8:] == 0xA5A5A5A5).all() and (sel[n:] == 0x5A).all() and (lb[n:] == 0x5A).all() and (cnt[1:] == 0xA5A5A5A5).all()


def mixed_state(n, seed=5):
    """a state in the middle of a path: throughputs around 1, some radiance, every seventh entry inactive, a reserved word to carry"""
    rng = np.random.default_rng(seed)
    st = np.zeros(n, T.PATH_STATE)
    st["throughput"], st["radiance"] = rng.uniform(0.05, 2.0, (n, 3)), rng.uniform(0, 3, (n, 3))
    st["active"], st["reserved"] = (np.arange(n) % 7 != 0), np.arange(n) * 3 + 1
    return st


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_single_steps_in_every_form(built, kind, grid):
    """A bounce-0 step from mrt_path_init's state in the grid, array and host-layout forms; the grid form also at bounce 2 (roulette)
    and at the last bounce from a state in the middle of a path."""
    ch = Chain(kind, *grid)
    run, lit = ch.run, ch.lit
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        fresh = P.init_state(n)
        out = Outputs(dev, n, np.zeros(n, T.PATH_STATE))
        ctx.path_init(out.d_state, n)
        same(dev.get(out.d_state, n, T.PATH_STATE), fresh)
        info = {}
        want = ch.want(fresh, 0, 4, info=info)
        assert (info["missed"].any() or kind != "soup") and (want[2] == B.LOBE_DIFFUSE).any() and (want[2] == B.LOBE_SPECULAR).any() and want[3] > 0
        ctx.path_grid_step(run.cam, run.w, run.h, ch.d_shits, lit.d_rows, ch.d_direct, out.d_state, ch.env, out.d_select, FRAME, 0, 4,
                           out.d_lobe, out.d_count, y0=run.y0, y1=run.y1)
        out.check(want)
        for bounce, last in ((2, 4), (3, 3), (1, 32)):
            st = mixed_state(n, bounce)
            info = {}
            want = ch.want(st, bounce, last, info=info)
            if bounce == 2:
                assert info["killed"].any() and info["survived"].any()
            o = Outputs(dev, n, st)
            ctx.path_grid_step(run.cam, run.w, run.h, ch.d_shits, lit.d_rows, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, bounce, last,
                               o.d_lobe, o.d_count, y0=run.y0, y1=run.y1)
            o.check(want)
            same(dev.get(o.d_state, n, T.PATH_STATE)[::7], st[::7])                # an inactive entry is not written
        # the array form on what mrt_cast read and wrote: the stream is seeded from the record's index
        d_rays = dev.put(run.rays)
        o = Outputs(dev, n, fresh)
        ctx.path_step(d_rays, ch.d_shits, lit.d_rows, n, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, 0, 4, o.d_lobe, o.d_count)
        o.check(ch.want(fresh, 0, 4, grid=False))
        # without the optional outputs
        o2 = Outputs(dev, n, fresh)
        ctx.path_step(d_rays, ch.d_shits, lit.d_rows, n, ch.d_direct, o2.d_state, ch.env, o2.d_select, FRAME, 0, 4)
        same(dev.get(o2.d_state, n, T.PATH_STATE), dev.get(o.d_state, n, T.PATH_STATE))
        same(dev.get(o2.d_select, n, np.uint8), dev.get(o.d_select, n, np.uint8))
        assert (dev.get(o2.d_lobe, n + 64, np.uint8) == 0x5A).all() and dev.get(o2.d_count, 1, np.uint32)[0] == 0
        # the reference's host layout
        hrays = po.make_host_rays(run.rays)
        d_hr, d_h44, d_s44 = dev.put(hrays), dev.alloc(n * 44), dev.alloc(n * 44)
        ctx.cast(d_hr, d_h44, count=n, flags=DEV | capi.FLAG_HOST_LAYOUT)
        d_rows44, d_mask44, d_dir44 = dev.alloc(n * 64), dev.alloc(16 * n), dev.alloc(n * 16)
        ctx.resolve_surfaces(d_hr, d_h44, n, d_rows44, d_out_hits=d_s44, flags=capi.FLAG_HOST_LAYOUT)
        ctx.cast_shadows(d_hr, d_h44, n, capi.shadow_lights(lit.lights), d_mask44, flags=capi.FLAG_HOST_LAYOUT)
        ctx.light_surfaces(d_hr, d_h44, d_rows44, n, lit.lights, d_dir44, d_mask44, None, flags=capi.FLAG_HOST_LAYOUT)
        rows44, s44, dir44 = dev.get(d_rows44, n, T.SURFACE64), dev.get(d_s44, n, T.HOST_HIT44), dev.get(d_dir44, n * 4, F).reshape(-1, 4)
        o = Outputs(dev, n, fresh)
        ctx.path_step(d_hr, d_s44, d_rows44, n, d_dir44, o.d_state, ch.env, o.d_select, FRAME, 0, 4, o.d_lobe, o.d_count, flags=capi.FLAG_HOST_LAYOUT)
        o.check(P.path_step(fresh, rows44, s44["prim_id"] != T.NO_HIT, s44["normal"], hrays["direction"], dir44, ch.env,
                            np.arange(n, dtype=np.uint64), FRAME, 0, 4))
    finally:
        ch.close()


def test_a_band_steps_what_the_whole_frame_steps(built):
    whole, band = Chain("room", 128, 96), Chain("room", 128, 96, 20, 70)
    try:
        got = []
        for ch in (whole, band):
            r = ch.run
            st = mixed_state(128 * 96, 9)[r.y0 * 128:r.y1 * 128]
            o = Outputs(r.dev, r.n, st)
            r.ctx.path_grid_step(r.cam, r.w, r.h, ch.d_shits, ch.lit.d_rows, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, 2, 4, o.d_lobe,
                                 o.d_count, y0=r.y0, y1=r.y1)
            got.append((r.dev.get(o.d_state, r.n, T.PATH_STATE), r.dev.get(o.d_select, r.n, np.uint8), r.dev.get(o.d_lobe, r.n, np.uint8)))
        for a, b in zip(got[0], got[1]):
            same(a[20 * 128:70 * 128], b)
    finally:
        whole.close()
        band.close()


# ---- the whole loop ---------------------------------------------------------------------------------------------------------------------

def cases_of(b, max_bounces, state_in, rows, hit, lobe, info):
    on = state_in["active"] != 0
    return {"miss at bounce 0": b == 0 and bool(info["missed"].any()), "miss at a later bounce": b > 0 and bool(info["missed"].any()),
            "invalid sample": bool(info["invalid"].any()), "roulette kill": bool(info["killed"].any()), "roulette survival": bool(info["survived"].any()),
            "diffuse lobe": bool((lobe == B.LOBE_DIFFUSE).any()), "specular lobe": bool((lobe == B.LOBE_SPECULAR).any()),
            "last-bounce stop": b == max_bounces and bool(info["stopped"].any()),
            "emissive hit": bool((on & hit & (rows["emission"] > 0).any(axis=1)).any()), "inactive entry passing through": b > 0 and bool((~on).any())}


def cpu_loop_cases(frame):
    """The loop on the CPU with oracle-traced records and the restatements: which cases occur for this frame number."""
    sc, shade, (w, h) = scene(LOOP_KIND), shade_data(LOOP_KIND), LOOP_GRID
    lights, env = light_list(LOOP_KIND)[:LOOP_LIGHTS], environment()
    n = w * h
    rays = po.grid_rays(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
    pixel = np.arange(n, dtype=np.uint64)
    state = P.init_state(n)
    seen = {c: False for c in CASES}
    for b in range(LOOP_BOUNCES + 1):
        hits = sc.oracle(rays)
        rows, pairs, shits = expected(rays, hits, shade)
        hit, p = hits["prim_id"] != -1, hit_point(rays, hits)
        mask = shadow_mask(sc, rays, hits, lights).reshape(LOOP_LIGHTS, n)
        direct = Lg.shade_linear(rows, hit, p, rays["direction"], lights, mask, None)[0]
        info = {}
        new, select, lobe, count = P.path_step(state, rows, hit, shits["normal"], rays["direction"], direct, env, pixel, frame, b, LOOP_BOUNCES, info)
        for c, v in cases_of(b, LOOP_BOUNCES, state, rows, hit, lobe, info).items():
            seen[c] |= v
        state = new
        if count == 0 or b == LOOP_BOUNCES:
            break
        rays = B.bounce_rays(rays["direction"], p, shits["normal"], hit, pixel, frame, P.first_draw(b), FAR, pairs[:, 0], pairs[:, 1], select)[0]
    return seen


def test_whole_loop_against_trace_frame(built):
    """init, then per bounce cast -> resolve -> shadows -> light with env = NULL -> step -> bounce cast with the step's select, every
    call ASYNC with one 4-byte read-back; then the finished frame in the five modes."""
    seen = cpu_loop_cases(FRAME)
    assert all(seen.values()), seen                                            # known to occur before anything runs on the device
    w, h = LOOP_GRID
    ch = Chain(LOOP_KIND, w, h)
    run, lit = ch.run, ch.lit
    ctx, dev, n = run.ctx, run.dev, run.n
    A = capi.FLAG_ASYNC
    try:
        lights, env = lit.lights[:LOOP_LIGHTS], ch.env
        shadow = capi.shadow_lights(lights)
        pairs = [(dev.alloc(n * 32), dev.alloc(n * 32)), (dev.alloc(n * 32), dev.alloc(n * 32))]   # (rays, records) of the odd and the even bounces
        d_rows, d_pairs, d_shits, d_mask, d_direct = dev.alloc(n * 64), dev.alloc(n * 8), dev.alloc(n * 32), dev.alloc(LOOP_LIGHTS * n), dev.alloc(n * 16)
        d_state, d_select, d_lobe, d_cast_lobe = dev.alloc(n * 32), dev.alloc(n), dev.alloc(n), dev.alloc(n)
        d_counts = dev.put(np.zeros(LOOP_BOUNCES + 1, np.uint32))
        ctx.path_init(d_state, n, flags=A)
        records, got = [], []
        rays_host = run.rays
        for b in range(LOOP_BOUNCES + 1):
            cur_rays, cur_hits = (None, run.d_hits) if b == 0 else pairs[b & 1]
            nxt_rays, nxt_hits = pairs[(b + 1) & 1]
            kw = dict(frame=FRAME, bounce=b, max_bounces=LOOP_BOUNCES, d_out_lobe=d_lobe, d_active_count=d_counts + 4 * b, flags=A)
            if b == 0:
                ctx.resolve_grid_surfaces(run.cam, w, h, cur_hits, d_rows, d_pairs, d_shits, flags=A)
                ctx.cast_grid_shadows(run.cam, w, h, cur_hits, shadow, d_mask, flags=A)
                ctx.light_grid_surfaces(run.cam, w, h, cur_hits, d_rows, lights, d_direct, d_mask, None, flags=A)
                ctx.path_grid_step(run.cam, w, h, d_shits, d_rows, d_direct, d_state, env, d_select, **kw)
            else:
                ctx.resolve_surfaces(cur_rays, cur_hits, n, d_rows, d_pairs, d_shits, flags=A)
                ctx.cast_shadows(cur_rays, cur_hits, n, shadow, d_mask, flags=A)
                ctx.light_surfaces(cur_rays, cur_hits, d_rows, n, lights, d_direct, d_mask, None, flags=A)
                ctx.path_step(cur_rays, d_shits, d_rows, n, d_direct, d_state, env, d_select, **kw)
            if b < LOOP_BOUNCES:
                bk = dict(frame=FRAME, first_draw=P.first_draw(b), t_max=FAR, d_select=d_select, d_surface=d_pairs, d_out_lobe=d_cast_lobe,
                          d_out_rays=nxt_rays, flags=A)
                if b == 0:
                    ctx.cast_grid_bounce(run.cam, w, h, d_shits, nxt_hits, **bk)
                else:
                    ctx.cast_bounce(cur_rays, d_shits, n, nxt_hits, **bk)
            ctx.synchronize()
            count = int(dev.get(d_counts + 4 * b, 1, np.uint32)[0])                 # the loop's one read-back; the rest is for the comparison
            shits = dev.get(d_shits, n, T.HIT32)
            records.append(dict(rows=dev.get(d_rows, n, T.SURFACE64), hit=shits["prim_id"] != -1, normal=shits["normal"],
                                direction=rays_host["direction"], direct=dev.get(d_direct, n * 4, F).reshape(-1, 4)))
            got.append((dev.get(d_state, n, T.PATH_STATE), dev.get(d_select, n, np.uint8), dev.get(d_lobe, n, np.uint8), count))
            if b < LOOP_BOUNCES:
                # agreement with the cast that follows: the same lobe wherever a ray was made, the placeholder everywhere else
                cast_lobe = dev.get(d_cast_lobe, n, np.uint8)
                rays_host = dev.get(nxt_rays, n, T.RAY32)
                nhits = dev.get(nxt_hits, n, T.HIT32)
                sel = got[-1][1] != 0
                np.testing.assert_array_equal(cast_lobe, got[-1][2])
                assert (cast_lobe[sel] != B.LOBE_NONE).all() and (cast_lobe[~sel] == B.LOBE_NONE).all()
                same(rays_host[~sel], np.repeat(B.H.PLACEHOLDER, int((~sel).sum())))
                assert (nhits["prim_id"][~sel] == -1).all() and (rays_host["t_max"][sel] == FAR).all()
            if count == 0:
                break
        want = P.trace_frame(iter(records), env, np.arange(n, dtype=np.uint64), FRAME, LOOP_BOUNCES)
        assert len(want) == len(got) == LOOP_BOUNCES + 1
        seen = {c: False for c in CASES}
        state_in = P.init_state(n)
        for b, (g, wnt, rec) in enumerate(zip(got, want, records)):
            np.testing.assert_array_equal(words(g[0]).reshape(-1, 8), words(wnt[0]).reshape(-1, 8), err_msg=f"state after bounce {b}")
            np.testing.assert_array_equal(g[1], wnt[1], err_msg=f"select of bounce {b}")
            np.testing.assert_array_equal(g[2], wnt[2], err_msg=f"lobe of bounce {b}")
            assert g[3] == wnt[3] == int(g[1].sum()), b
            info = {}
            P.path_step(state_in, rec["rows"], rec["hit"], rec["normal"], rec["direction"], rec["direct"], env, np.arange(n, dtype=np.uint64), FRAME, b,
                        LOOP_BOUNCES, info)
            for c, v in cases_of(b, LOOP_BOUNCES, state_in, rec["rows"], rec["hit"], g[2], info).items():
                seen[c] |= v
            state_in = g[0]
        assert all(seen.values()), seen
        assert (got[-1][0]["active"] == 0).all() and got[-1][3] == 0
        d_rgba = dev.put(np.full(n * 4 + 64, -7.5, F))
        for mode in range(5):
            ctx.path_finish(d_state, n, d_rgba, mode, flags=A)
            ctx.synchronize()
            out = dev.get(d_rgba, n * 4 + 64, F)
            np.testing.assert_array_equal(words(out[:n * 4].reshape(-1, 4)), words(P.path_finish(got[-1][0], mode)), err_msg=f"mode {mode}")
            assert (out[n * 4:] == F(-7.5)).all()
        assert np.isfinite(P.path_finish(got[-1][0], 0)).all() and (P.path_finish(got[-1][0], 0)[:, :3] > 0).any()
    finally:
        ch.close()


@pytest.mark.parametrize("count", [1, 255, 257, 2 ** 16 + 1])
def test_array_counts_and_guards(built, count):
    """The array form on the first `count` records of a 257 x 256 grid at bounce 2; init and finish on as many entries: guard words
    behind every output keep their pattern and every input is read only."""
    ch = Chain("soup", 257, 256)
    run, lit = ch.run, ch.lit
    ctx, dev = run.ctx, run.dev
    try:
        d_rays = dev.put(run.rays)
        st = mixed_state(count, count)
        o = Outputs(dev, count, st)
        inputs = ((lit.d_rows, run.n * 64), (ch.d_shits, run.n * 32), (d_rays, run.n * 32), (ch.d_direct, run.n * 16))
        before = [dev.get(p, k, np.uint8) for p, k in inputs]
        ctx.path_step(d_rays, ch.d_shits, lit.d_rows, count, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, 2, 4, o.d_lobe, o.d_count)
        o.check(P.path_step(st, lit.rows[:count], lit.hit[:count], ch.shits["normal"][:count], run.rays["direction"][:count], ch.direct[:count], ch.env,
                            np.arange(count, dtype=np.uint64), FRAME, 2, 4))
        for a, (p, k) in zip(before, inputs):
            np.testing.assert_array_equal(a, dev.get(p, k, np.uint8))
        got_state = dev.get(o.d_state, count, T.PATH_STATE)
        d_rgba = dev.put(np.full((count + 64) * 4, -7.5, F))
        ctx.path_finish(o.d_state, count, d_rgba, 3)
        out = dev.get(d_rgba, (count + 64) * 4, F)
        np.testing.assert_array_equal(words(out[:count * 4].reshape(-1, 4)), words(P.path_finish(got_state, 3)))
        assert (out[count * 4:] == F(-7.5)).all()
        same(dev.get(o.d_state, count, T.PATH_STATE), got_state)                 # finish reads only
        ctx.path_init(o.d_state, count)
        raw = dev.get(o.d_state, count * 8 + 64, np.uint32)
        same(raw[:count * 8], P.init_state(count))
        assert (raw[count * 8:] == 0xA5A5A5A5).all()
    finally:
        ch.close()


def test_async_then_synchronize(built):
    ch = Chain("soup", 100, 77)
    run, lit = ch.run, ch.lit
    ctx, dev, n = run.ctx, run.dev, run.n
    try:
        d_rays = dev.put(run.rays)
        a, b = Outputs(dev, n, np.zeros(n, T.PATH_STATE)), Outputs(dev, n, np.zeros(n, T.PATH_STATE))
        d_rgba = dev.alloc(n * 16)
        A = capi.FLAG_ASYNC
        ctx.path_init(a.d_state, n, flags=A)
        ctx.path_init(b.d_state, n, flags=A)
        ctx.path_grid_step(run.cam, run.w, run.h, ch.d_shits, lit.d_rows, ch.d_direct, a.d_state, ch.env, a.d_select, FRAME, 0, 0, a.d_lobe, a.d_count, flags=A)
        ctx.path_step(d_rays, ch.d_shits, lit.d_rows, n, ch.d_direct, b.d_state, ch.env, b.d_select, FRAME, 0, 0, b.d_lobe, b.d_count, flags=A)
        ctx.path_finish(a.d_state, n, d_rgba, 2, flags=A)
        ctx.synchronize()
        want = ch.want(P.init_state(n), 0, 0)
        assert want[3] == 0                                                     # max_bounces 0: direct light only, every path ends
        a.check(want)
        b.check(want)
        np.testing.assert_array_equal(words(dev.get(d_rgba, n * 4, F).reshape(-1, 4)), words(P.path_finish(want[0], 2)))
    finally:
        ch.close()


@pytest.mark.parametrize("kind", ["soup", "room_tl"])
def test_step_with_nothing_resident(built, kind):
    """No shade data: the default material and the face normal everywhere, no emission; the same calls."""
    ch = Chain(kind, 100, 77, shade=False)
    run = ch.run
    try:
        assert (ch.lit.rows["material"] == T.DEFAULT_MATERIAL).all()
        for bounce in (0, 2):
            st = mixed_state(run.n, 20 + bounce)
            o = Outputs(run.dev, run.n, st)
            run.ctx.path_grid_step(run.cam, run.w, run.h, ch.d_shits, ch.lit.d_rows, ch.d_direct, o.d_state, ch.env, o.d_select, FRAME, bounce, 4,
                                   o.d_lobe, o.d_count)
            o.check(ch.want(st, bounce, 4))
    finally:
        ch.close()


def test_refusals_count_zero_and_pending(built):
    """Every refusal, with and without a scene, before anything is written and before the pending test; count == 0 is OK and writes
    nothing; no scene is needed."""
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
        env = np.zeros(1, T.ENVIRONMENT)
        env[0] = environment()
        direct = np.random.default_rng(3).uniform(0, 2, (n, 4)).astype(F)
        state = mixed_state(n, 1)
        d_rays, d_hits, d_rows, d_direct = dev.put(rays), dev.put(hits), dev.put(rows), dev.put(direct)
        d_state, d_select, d_lobe, d_count = dev.put(state), dev.put(np.full(n, 0x5A, np.uint8)), dev.put(np.full(n, 0x5A, np.uint8)), dev.put(np.zeros(4, np.uint32))
        pattern = np.full(n * 4, -7.5, F)
        d_rgba = dev.put(pattern)
        R, Hp, Rw = (C.c_void_p(x) for x in (d_rays, d_hits, d_rows))

        def desc(frame=FRAME, bounce=2, max_bounces=4, direct=d_direct, st=d_state, e=env, select=d_select, lobe=d_lobe, count=d_count):
            return capi.PathStepDesc(frame, bounce, max_bounces, 0, direct, st, None if e is None else e.ctypes.data_as(C.c_void_p).value, select, lobe, count)

        def arr(rays=R, hits=Hp, rows=Rw, count=n, flags=0, d=True, **kw):
            dd = desc(**kw)
            return L.mrt_path_step(ctx.h, rays, hits, rows, count, C.byref(dd) if d else None, flags)

        def grid(hits=Hp, rows=Rw, flags=0, camera=cam, y0=0, y1=h, d=True, **kw):
            dd = desc(**kw)
            return L.mrt_path_grid_step(ctx.h, None if camera is None else C.byref(camera), w, h, y0, y1, hits, rows, C.byref(dd) if d else None, flags)

        def bad_env(word):
            e = env.copy()
            e.view(F)[word] = np.nan
            return e

        def bad_calls():
            common = [dict(hits=None), dict(rows=None), dict(d=False), dict(direct=None), dict(st=None), dict(e=None), dict(select=None),
                      dict(bounce=5), dict(bounce=1, max_bounces=0), dict(frame=T.PATH_MAX_FRAME + 1), dict(frame=0xFFFFFFFF),
                      dict(max_bounces=T.PATH_MAX_BOUNCES + 1), dict(bounce=0xFFFFFFFF, max_bounces=0xFFFFFFFF), dict(e=bad_env(0)), dict(e=bad_env(12))]
            for kw in common + [dict(rays=None)]:
                assert arr(**kw) == capi.ERR_INVALID, kw
            for kw in common + [dict(camera=None), dict(y0=10, y1=5), dict(y1=h + 1), dict(flags=capi.FLAG_HOST_LAYOUT)]:
                assert grid(**kw) == capi.ERR_INVALID, kw
            for fl in (capi.FLAG_BOOL_OUT, capi.FLAG_TOKEN_OUT, capi.FLAG_COHERENT, capi.FLAG_FORCE_SORT, capi.FLAG_RAYS_ON_DEVICE, 1 << 20):
                assert arr(flags=fl) == capi.ERR_INVALID and grid(flags=fl) == capi.ERR_INVALID, fl
                assert L.mrt_path_init(ctx.h, d_state, n, fl) == capi.ERR_INVALID and L.mrt_path_finish(ctx.h, d_state, n, 0, d_rgba, fl) == capi.ERR_INVALID
            assert L.mrt_path_init(ctx.h, None, n, 0) == capi.ERR_INVALID and L.mrt_path_init(ctx.h, d_state, n, capi.FLAG_HOST_LAYOUT) == capi.ERR_INVALID
            assert L.mrt_path_finish(ctx.h, None, n, 0, d_rgba, 0) == capi.ERR_INVALID and L.mrt_path_finish(ctx.h, d_state, n, 0, None, 0) == capi.ERR_INVALID
            assert L.mrt_path_finish(ctx.h, d_state, n, 5, d_rgba, 0) == capi.ERR_INVALID and L.mrt_path_finish(ctx.h, d_state, n, 0xFFFFFFFF, d_rgba, 0) == capi.ERR_INVALID
            assert arr(frame=T.PATH_MAX_FRAME, count=0) == capi.MRT_OK and arr(bounce=32, max_bounces=32, count=0) == capi.MRT_OK

        def untouched():
            return (same(dev.get(d_state, n, T.PATH_STATE), state) is None and (dev.get(d_select, n, np.uint8) == 0x5A).all()
                    and (dev.get(d_lobe, n, np.uint8) == 0x5A).all() and (dev.get(d_count, 4, np.uint32) == 0).all() and (dev.get(d_rgba, n * 4, F) == F(-7.5)).all())

        bad_calls()                                   # no scene
        assert arr(count=0) == capi.MRT_OK and grid(y0=10, y1=10) == capi.MRT_OK
        assert L.mrt_path_init(ctx.h, d_state, 0, 0) == capi.MRT_OK and L.mrt_path_finish(ctx.h, d_state, 0, 4, d_rgba, 0) == capi.MRT_OK
        assert untouched()
        sc.upload(ctx)
        upload(ctx, shade_data("soup"))
        bad_calls()
        assert untouched()
        ctx.submit(rays)
        assert arr() == capi.ERR_PENDING and grid() == capi.ERR_PENDING
        assert L.mrt_path_init(ctx.h, d_state, n, 0) == capi.ERR_PENDING and L.mrt_path_finish(ctx.h, d_state, n, 0, d_rgba, 0) == capi.ERR_PENDING
        assert arr(bounce=5) == capi.ERR_INVALID and L.mrt_path_finish(ctx.h, d_state, n, 5, d_rgba, 0) == capi.ERR_INVALID   # the checks come first
        ctx.collect()
        assert untouched()
        # and the good call, no scene needed for it either: the array form on the oracle's records
        want = P.path_step(state, rows, hits["prim_id"] != -1, hits["normal"], rays["direction"], direct, env[0], np.arange(n, dtype=np.uint64), FRAME, 2, 4)
        assert arr() == capi.MRT_OK
        same(dev.get(d_state, n, T.PATH_STATE), want[0])
        np.testing.assert_array_equal(dev.get(d_select, n, np.uint8), want[1])
        np.testing.assert_array_equal(dev.get(d_lobe, n, np.uint8), want[2])
        assert dev.get(d_count, 1, np.uint32)[0] == want[3]
    finally:
        dev.free()
        ctx.close()


def test_primary_grid_unaffected_by_path_calls(built):
    """A renderer's frames: the primary grid with and without the path calls between frames -- the same kernel sequence, the same records."""
    sc = scene("room")
    w, h = 640, 480
    n = w * h
    runs = []
    for path in (False, True):
        ctx = capi.Context(0)
        dev = Dev(ctx)
        try:
            sc.upload(ctx)
            upload(ctx, shade_data("room"))
            cam = capi.camera_look(sc.cam[0], sc.cam[1], w, h, sc.cam[2])
            kernels, records = [], []
            d_hits, d_rows, d_shits, d_direct = dev.alloc(n * 32), dev.alloc(n * 64), dev.alloc(n * 32), dev.put(np.full(n * 4, 0.25, F))
            d_state, d_select, d_count, d_rgba = dev.alloc(n * 32), dev.alloc(n), dev.put(np.zeros(1, np.uint32)), dev.alloc(n * 16)
            for f in range(8):
                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                kernels.append((ctx.stats()["last_kernel"], ctx.last_kernel_variant()))
                records.append(dev.get(d_hits, n, T.HIT32).view(np.uint32))
                if path:
                    fl = capi.FLAG_ASYNC if f & 1 else 0
                    ctx.path_init(d_state, n, flags=fl)
                    ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows, d_out_hits=d_shits)
                    ctx.path_grid_step(cam, w, h, d_shits, d_rows, d_direct, d_state, environment(), d_select, f, 0, 0, d_active_count=d_count, flags=fl)
                    ctx.path_finish(d_state, n, d_rgba, f % 5, flags=fl)
            runs.append((kernels, records))
        finally:
            dev.free()
            ctx.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)
