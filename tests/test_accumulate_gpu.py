"""mrt_accumulate: the running mean of progressive frames and its 8-bit image on the device, held to the numpy float32 restatement
(messyerraytracer_amd/accumulate.py; pinned to the reference by test_accumulate_cpu.py) byte for byte -- the accumulator as uint32
words, the image as bytes, a NaN as a NaN.  The recorded sequences; counts at the workgroup's edge with every n_prior; bytes asked for
and not; the two fused sources against the finishing passes, on the device and in numpy; a rasterised and a path-traced progressive
frame whose camera mrt_accum_begin_frame jitters; ASYNC; refusals; primary grids unaffected.  Guard words behind every output."""
import ctypes as C
import os

import numpy as np
import pytest

from messyerraytracer_amd import accumulate as A
from messyerraytracer_amd import capi, types as T
from messyerraytracer_amd import channels as Ch
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import path as P
from oracle import pyoracle as po
from test_hemisphere_gpu import Dev, hit_point, same, scene
from test_lighting_gpu import environment, light_list
from test_surface_gpu import expected, shade_data, upload

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
PATTERN = 0xA5A5A5A5
FAR = F(1e30)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accumulate_reference.npz")
W, H = 64, 48
ROOM_ORIGIN, ROOM_FWD, ROOM_FOV = (0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_floats(got, want, what=""):
    """bit for bit, but a NaN for a NaN whatever its payload"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what
    np.testing.assert_array_equal(words(got)[~nan], words(want)[~nan], err_msg=what)


class Out:
    """an accumulator and an image on the device, a guard behind each"""

    def __init__(self, dev, n, acc=None, bytes8=True):
        self.dev, self.n = dev, n
        first = np.full(n * 4, PATTERN, np.uint32) if acc is None else words(np.ascontiguousarray(acc, dtype=F)).reshape(-1)
        self.d_acc = dev.put(np.concatenate([first, np.full(GUARD, PATTERN, np.uint32)]))
        self.d_rgba8 = dev.put(np.full(n + GUARD, PATTERN, np.uint32)) if bytes8 else None

    def read(self):
        n = self.n
        got = self.dev.get(self.d_acc, n * 4 + GUARD, np.uint32)
        assert (got[n * 4:] == PATTERN).all()
        acc = got[:n * 4].view(F).reshape(-1, 4)
        if self.d_rgba8 is None:
            return acc, None
        got8 = self.dev.get(self.d_rgba8, n + GUARD, np.uint32)
        assert (got8[n:] == PATTERN).all()
        return acc, got8[:n].view(np.uint8).reshape(-1, 4)

    def check(self, want, what="", exact=False):
        acc, got8 = self.read()
        if exact:
            np.testing.assert_array_equal(words(acc), words(want), err_msg=what)
        else:
            same_floats(acc, want, what)
        if got8 is not None:
            np.testing.assert_array_equal(got8, Ch.to_rgba8(want), err_msg=what + " bytes")

    def untouched(self):
        return (self.dev.get(self.d_acc, self.n * 4 + GUARD, np.uint32) == PATTERN).all() and (
            self.d_rgba8 is None or (self.dev.get(self.d_rgba8, self.n + GUARD, np.uint32) == PATTERN).all())


@pytest.fixture(scope="module")
def gpu(built):
    ctx = capi.Context(0)
    dev = Dev(ctx)
    yield ctx, dev
    dev.free()
    ctx.close()


def test_recorded_sequences(gpu):
    """1. RGBA source on the fixture's sequences: the accumulator and the bytes after every sample equal the recording."""
    ctx, dev = gpu
    g = np.load(GOLDEN)
    src, want, want8 = g["a_src"], g["a_acc"], g["a_bytes"]
    n = src.shape[1] // 4
    assert np.isnan(want).any() and np.isinf(want).any() and (words(src[0]) == 0x80000000).any()
    out = Out(dev, n)
    d_src = dev.alloc(n * 16)
    for k in range(src.shape[0]):
        ctx.h2d(d_src, src[k])
        ctx.accumulate(capi.ACCUM_SRC_RGBA, d_src, n, out.d_acc, k, out.d_rgba8)
        acc, got8 = out.read()
        same_floats(acc.reshape(-1), want[k], f"sample {k}")
        np.testing.assert_array_equal(got8.reshape(-1), want8[k], err_msg=f"bytes after sample {k}")


def _samples(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-0.25, 1.25, (n, 4)).astype(F)
    s[rng.integers(0, n, max(n // 16, 1)), rng.integers(0, 4)] = np.nan
    s[0, 1], s[n - 1, 2] = -0.0, np.inf
    return s


@pytest.mark.parametrize("count", [1, 255, 256, 257, 2 ** 16 + 3])
def test_counts_at_the_workgroup_edge_and_every_n_prior(gpu, count):
    """2. The outputs end where the count ends; n_prior 0, 1, 2, 4095 and the largest."""
    ctx, dev = gpu
    acc0, s = _samples(count, 1), _samples(count, 2)
    d_src = dev.put(s)
    for n_prior in (0, 1, 2, 4095, 0x7FFFFFFE):
        out = Out(dev, count, acc0)
        ctx.accumulate(capi.ACCUM_SRC_RGBA, d_src, count, out.d_acc, n_prior, out.d_rgba8)
        out.check(A.accumulate(acc0, s, n_prior), f"n_prior {n_prior}", exact=n_prior == 0)
    assert (words(A.accumulate(acc0, s, 1)) != words(A.accumulate(acc0, s, 2))).any()
    dev.free()
    dev.ptrs.clear()


def test_bytes_optional_source_only_read_and_first_copy(gpu):
    """3. d_rgba8 null and non-null; the source is only read; n_prior == 0 copies NaN payloads and -0 bits unchanged."""
    ctx, dev = gpu
    n = 1000
    s = _samples(n, 3)
    words(s)[5, 0], words(s)[6, 3], words(s)[7, 2] = 0xFFC12345, 0x7F800001, 0x80000000   # two payloads and a -0
    src_guarded = np.concatenate([words(s).reshape(-1), np.full(GUARD, PATTERN, np.uint32)])
    d_src = dev.put(src_guarded)
    for bytes8 in (True, False):
        out = Out(dev, n, bytes8=bytes8)
        ctx.accumulate(capi.ACCUM_SRC_RGBA, d_src, n, out.d_acc, 0, out.d_rgba8)
        out.check(s, "first copy", exact=True)
        acc1 = out.read()[0].copy()
        s2 = _samples(n, 4)
        d_s2 = dev.put(s2)
        ctx.accumulate(capi.ACCUM_SRC_RGBA, d_s2, n, out.d_acc, 1, out.d_rgba8)
        out.check(A.accumulate(acc1, s2, 1), "second sample")
        same(dev.get(d_s2, n * 4, F), s2.reshape(-1))
    same(dev.get(d_src, n * 4 + GUARD, np.uint32), src_guarded)


@pytest.mark.parametrize("mode", range(5))
def test_fused_sources_equal_finish_then_rgba(gpu, mode):
    """4. LIT and PATH_STATE equal mrt_finish_color / mrt_path_finish followed by the RGBA form: on the device, and in numpy."""
    ctx, dev = gpu
    n = 2 * 256 + 77
    rng = np.random.default_rng(40 + mode)
    lit = np.zeros((n, 4), F)
    lit[:, :3] = rng.uniform(0, 4, (n, 3)).astype(F) * rng.choice(F([0, 1e-3, 1, 8, 40]), (n, 1))
    lit[:, 3] = rng.integers(0, 2, n)
    state = P.init_state(n)
    state["radiance"], state["throughput"], state["reserved"] = lit[:, :3], rng.uniform(0, 2, (n, 3)), np.arange(n)
    acc0 = rng.uniform(0, 1, (n, 4)).astype(F)
    d_lit, d_state, d_fin = dev.put(lit), dev.put(state), dev.alloc(n * 16)
    for kind, d_src, host in ((capi.ACCUM_SRC_LIT, d_lit, lit), (capi.ACCUM_SRC_PATH_STATE, d_state, state)):
        if kind == capi.ACCUM_SRC_LIT:
            ctx.finish_color(d_src, n, d_fin, None, tonemap_mode=mode)
        else:
            ctx.path_finish(d_src, n, d_fin, mode)
        fin = dev.get(d_fin, n * 4, F).reshape(-1, 4)
        np.testing.assert_array_equal(words(fin), words(A.sample(kind, host, mode)))
        for n_prior in (0, 1, 6):
            fused, two = Out(dev, n, acc0), Out(dev, n, acc0)
            ctx.accumulate(kind, d_src, n, fused.d_acc, n_prior, fused.d_rgba8, tonemap_mode=mode)
            ctx.accumulate(capi.ACCUM_SRC_RGBA, d_fin, n, two.d_acc, n_prior, two.d_rgba8)
            want, want8 = A.accumulate_frame(acc0, kind, host, n_prior, mode)
            fused.check(want, f"kind {kind} n_prior {n_prior}", exact=True)
            two.check(want, f"kind {kind} n_prior {n_prior}, two calls", exact=True)
            np.testing.assert_array_equal(fused.read()[1], want8)
        same(dev.get(d_src, host.nbytes // 4, np.uint32), words(host).reshape(-1))       # only read
    dev.free()
    dev.ptrs.clear()


def look_basis(fwd):
    """row-major camera basis whose -z column looks along fwd, y up"""
    f = np.asarray(fwd, np.float64) / np.linalg.norm(fwd)
    z = -f
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1).astype(F)


class Room:
    """synth.room() with shade data resident and a RayCamera over a W x H grid"""

    def __init__(self):
        self.sc = scene("room")
        self.ctx = capi.Context(0)
        self.dev = Dev(self.ctx)
        self.sc.upload(self.ctx)
        self.shade = shade_data("room")
        upload(self.ctx, self.shade)
        self.lights, self.env = light_list("room")[:4], environment()
        self.n = W * H
        dev, n = self.dev, self.n
        self.d_hits, self.d_rows, self.d_mask, self.d_lit = dev.alloc(n * 32), dev.alloc(n * 64), dev.alloc(4 * n), dev.alloc(n * 16)

    def camera(self, origin, basis, jitter):
        jitter = (float(jitter[0]), float(jitter[1]))
        return capi.ray_camera(origin, basis, W, H, ROOM_FOV, jitter=jitter), po.ray_camera_rays(origin, basis, W, H, ROOM_FOV, jitter=jitter)

    def close(self):
        self.dev.free()
        self.ctx.close()


def test_a_rasterised_progressive_frame(built):
    """5. Four frames jittered by mrt_accum_begin_frame: cast -> resolve -> shadows -> light -> mrt_accumulate(LIT); the mean and its
    bytes equal the numpy chain; then a camera move restarts the mean."""
    room = Room()
    ctx, dev, n = room.ctx, room.dev, room.n
    try:
        st, ref = capi.accum_state(True, 64), A.new_state(True, 64)
        out = Out(dev, n)
        want = None
        basis = look_basis(ROOM_FWD)
        jitters = []
        for f, origin in enumerate([ROOM_ORIGIN] * 4 + [(0.25, 3.0, 4.6)] * 2):
            capi.accum_begin_frame(st, origin, basis)
            A.begin_frame(ref, origin, basis)
            assert (st.sample_index, F(st.jitter_x), F(st.jitter_y)) == (ref["sample_index"], ref["jitter"][0], ref["jitter"][1])
            assert st.sample_index == (f if f < 4 else f - 4)
            jitters.append((st.jitter_x, st.jitter_y))
            cam, rays = room.camera(origin, basis, (st.jitter_x, st.jitter_y))
            assert (cam.jitter_x, cam.jitter_y) == (st.jitter_x, st.jitter_y)
            ctx.cast_grid(cam, W, H, hits=room.d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
            ctx.resolve_grid_surfaces(cam, W, H, room.d_hits, room.d_rows)
            ctx.cast_grid_shadows(cam, W, H, room.d_hits, capi.shadow_lights(room.lights), room.d_mask)
            ctx.light_grid_surfaces(cam, W, H, room.d_hits, room.d_rows, room.lights, room.d_lit, room.d_mask, room.env)
            capi.accum_end_frame(st, n)
            A.end_frame(ref, n)
            assert (st.accumulate, st.n_prior, st.count) == (ref["accumulate"], ref["n_prior"], ref["count"]) == (1, st.sample_index, st.sample_index + 1)
            ctx.accumulate(capi.ACCUM_SRC_LIT, room.d_lit, n, out.d_acc, st.n_prior, out.d_rgba8, tonemap_mode=3)
            # the numpy chain on the device's records and shadow mask
            hits, mask = dev.get(room.d_hits, n, T.HIT32), dev.get(room.d_mask, 4 * n, np.uint8).reshape(4, n)
            hit = hits["prim_id"] != -1
            rows = expected(rays, hits, room.shade)[0]
            lit = Lg.shade_linear(rows, hit, hit_point(rays, hits), rays["direction"], room.lights, mask, room.env)[0]
            np.testing.assert_array_equal(words(dev.get(room.d_lit, n * 4, F).reshape(-1, 4)), words(lit), err_msg=f"lit frame {f}")
            before = want
            want, _ = A.accumulate_frame(want, A.SRC_LIT, lit, ref["n_prior"], 3)
            out.check(want, f"frame {f}", exact=True)
            if f == 4:                                                                     # the move: the mean is the new frame alone
                np.testing.assert_array_equal(words(want), words(Ch.finish_color(lit, 3)))
                assert (words(want) != words(before)).any()
            elif f:
                assert (words(want) != words(before)).any() and (words(want) != words(Ch.finish_color(lit, 3))).any()
        assert len(set(jitters[:4])) == 4 and jitters[4] == jitters[0] and (want[:, 3] == 1).all() and np.isfinite(want).all()
    finally:
        room.close()


def test_a_path_traced_progressive_frame(built):
    """6. Three samples with frame = sample_index and two bounces through the path calls, each ended by mrt_accumulate(PATH_STATE)."""
    room = Room()
    ctx, dev, n = room.ctx, room.dev, room.n
    bounces = 2
    try:
        st = capi.accum_state(True, 64)
        out = Out(dev, n)
        basis = look_basis(ROOM_FWD)
        shadow = capi.shadow_lights(room.lights)
        pairs = [(dev.alloc(n * 32), dev.alloc(n * 32)), (dev.alloc(n * 32), dev.alloc(n * 32))]
        d_pairs, d_shits, d_direct = dev.alloc(n * 8), dev.alloc(n * 32), dev.alloc(n * 16)
        d_state, d_select = dev.alloc(n * 32), dev.alloc(n)
        want = None
        finished = []
        for s in range(3):
            capi.accum_begin_frame(st, ROOM_ORIGIN, basis)
            frame = st.sample_index
            assert frame == s
            cam, rays_host = room.camera(ROOM_ORIGIN, basis, (st.jitter_x, st.jitter_y))
            ctx.cast_grid(cam, W, H, hits=room.d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
            ctx.path_init(d_state, n)
            records = []
            for b in range(bounces + 1):
                cur_rays, cur_hits = (None, room.d_hits) if b == 0 else pairs[b & 1]
                nxt_rays, nxt_hits = pairs[(b + 1) & 1]
                kw = dict(frame=frame, bounce=b, max_bounces=bounces)
                if b == 0:
                    ctx.resolve_grid_surfaces(cam, W, H, cur_hits, room.d_rows, d_pairs, d_shits)
                    ctx.cast_grid_shadows(cam, W, H, cur_hits, shadow, room.d_mask)
                    ctx.light_grid_surfaces(cam, W, H, cur_hits, room.d_rows, room.lights, d_direct, room.d_mask, None)
                    ctx.path_grid_step(cam, W, H, d_shits, room.d_rows, d_direct, d_state, room.env, d_select, **kw)
                else:
                    ctx.resolve_surfaces(cur_rays, cur_hits, n, room.d_rows, d_pairs, d_shits)
                    ctx.cast_shadows(cur_rays, cur_hits, n, shadow, room.d_mask)
                    ctx.light_surfaces(cur_rays, cur_hits, room.d_rows, n, room.lights, d_direct, room.d_mask, None)
                    ctx.path_step(cur_rays, d_shits, room.d_rows, n, d_direct, d_state, room.env, d_select, **kw)
                shits = dev.get(d_shits, n, T.HIT32)
                records.append(dict(rows=dev.get(room.d_rows, n, T.SURFACE64), hit=shits["prim_id"] != -1, normal=shits["normal"],
                                    direction=rays_host["direction"], direct=dev.get(d_direct, n * 4, F).reshape(-1, 4)))
                if b < bounces:
                    bk = dict(frame=frame, first_draw=P.first_draw(b), t_max=FAR, d_select=d_select, d_surface=d_pairs, d_out_rays=nxt_rays)
                    if b == 0:
                        ctx.cast_grid_bounce(cam, W, H, d_shits, nxt_hits, **bk)
                    else:
                        ctx.cast_bounce(cur_rays, d_shits, n, nxt_hits, **bk)
                    rays_host = dev.get(nxt_rays, n, T.RAY32)
            state = P.trace_frame(iter(records), room.env, np.arange(n, dtype=np.uint64), frame, bounces)[-1][0]
            np.testing.assert_array_equal(words(dev.get(d_state, n, T.PATH_STATE)).reshape(-1, 8), words(state).reshape(-1, 8), err_msg=f"state of sample {s}")
            capi.accum_end_frame(st, n)
            assert (st.accumulate, st.n_prior) == (1, s)
            ctx.accumulate(capi.ACCUM_SRC_PATH_STATE, d_state, n, out.d_acc, st.n_prior, out.d_rgba8, tonemap_mode=1)
            want, _ = A.accumulate_frame(want, A.SRC_PATH_STATE, state, s, 1)
            out.check(want, f"sample {s}", exact=True)
            same(dev.get(d_state, n, T.PATH_STATE), state)                                 # only read
            finished.append(P.path_finish(state, 1))
        assert (words(finished[0]) != words(finished[1])).any() and (words(finished[1]) != words(finished[2])).any()   # the samples differ
        assert np.isfinite(want).all() and (want[:, :3] > 0).any() and (words(want) != words(finished[2])).any()
    finally:
        room.close()


def test_async_then_synchronize(gpu):
    """7. MRT_FLAG_ASYNC, three frames queued, then mrt_synchronize: the same bytes."""
    ctx, dev = gpu
    n = 777
    frames = [_samples(n, 10 + k) for k in range(3)]
    d_frames = [dev.put(f) for f in frames]
    a, b = Out(dev, n), Out(dev, n)
    for k in range(3):
        ctx.accumulate(capi.ACCUM_SRC_RGBA, d_frames[k], n, a.d_acc, k, a.d_rgba8, flags=capi.FLAG_ASYNC)
    ctx.synchronize()
    for k in range(3):
        ctx.accumulate(capi.ACCUM_SRC_RGBA, d_frames[k], n, b.d_acc, k, b.d_rgba8)
    want = None
    for k in range(3):
        want = A.accumulate(want, frames[k], k)
    a.check(want, "async")
    b.check(want, "blocking")
    np.testing.assert_array_equal(a.read()[1], b.read()[1])


def test_refusals_count_zero_pending_and_primary_grids(built):
    """8. Every refusal by its message and in order, before anything is written; count == 0 is OK and writes nothing; a pending dispatch;
    a primary grid cast before and after is unaffected."""
    L = capi.load()
    L.mrt_last_error.restype = C.c_char_p
    sc = scene("soup")
    w, h = 100, 77
    n = w * h
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        o, f, fov = sc.cam
        cam = capi.camera_look(o, f, w, h, fov)
        rays = po.grid_rays(o, f, w, h, fov)
        sc.upload(ctx)
        first = ctx.cast_grid(cam, w, h)
        kernel = (ctx.stats()["last_kernel"], ctx.last_kernel_variant())
        out = Out(dev, n)
        s = _samples(n, 20)
        d_src = dev.put(s)

        def call(kind=0, src=d_src, count=n, mode=0, n_prior=0, acc=out.d_acc, rgba8=out.d_rgba8, flags=0):
            return L.mrt_accumulate(ctx.h, kind, src, count, mode, n_prior, acc, rgba8, flags)

        def refused(word, **kw):
            return call(**kw) == capi.ERR_INVALID and word in L.mrt_last_error(ctx.h)

        assert refused(b"null", src=None) and refused(b"null", acc=None)
        for fl in (capi.FLAG_BOOL_OUT, capi.FLAG_TOKEN_OUT, capi.FLAG_COHERENT, capi.FLAG_FORCE_SORT, capi.FLAG_RAYS_ON_DEVICE, capi.FLAG_HOST_LAYOUT, 1 << 20):
            assert refused(b"flag", flags=fl), fl
        assert refused(b"source_kind", kind=3) and refused(b"source_kind", kind=0xFFFFFFFF)
        assert refused(b"tonemap", kind=1, mode=5) and refused(b"tonemap", kind=2, mode=5)
        assert refused(b"n_prior", n_prior=0x7FFFFFFF) and refused(b"n_prior", n_prior=0xFFFFFFFF)
        assert refused(b"d_source", acc=d_src)
        assert refused(b"overflow", count=1 << 59) and refused(b"overflow", count=(1 << 64) - 1)
        # the order: each call is wrong in everything the later checks look at
        worst = dict(kind=9, mode=9, n_prior=0xFFFFFFFF, acc=d_src, count=(1 << 64) - 1)
        assert refused(b"null", **{**worst, "src": None}, flags=1 << 20)
        assert refused(b"flag", **worst, flags=1 << 20)
        assert refused(b"source_kind", **worst)
        assert refused(b"tonemap", **{**worst, "kind": 2})
        assert refused(b"n_prior", **{**worst, "kind": 2, "mode": 4})
        assert refused(b"d_source", **{**worst, "kind": 2, "mode": 4, "n_prior": 7})
        assert refused(b"overflow", **{**worst, "kind": 2, "mode": 4, "n_prior": 7, "acc": out.d_acc})
        assert call(count=0) == capi.MRT_OK and call(kind=2, count=0, mode=4, n_prior=9) == capi.MRT_OK
        assert out.untouched()
        # a pending dispatch
        ctx.submit(rays)
        assert call() == capi.ERR_PENDING and call(kind=2, mode=3, n_prior=5) == capi.ERR_PENDING
        assert out.untouched()
        ctx.collect()
        stats = ctx.stats()
        assert call(mode=77) == capi.MRT_OK                                                # RGBA: the mode is not looked at
        out.check(s, "after the refusals", exact=True)
        assert call(n_prior=1, flags=capi.FLAG_ASYNC) == capi.MRT_OK
        ctx.synchronize()
        out.check(A.accumulate(s, s, 1), "a second frame")
        # the scene, the statistics and the next primary grid are as they were
        after = ctx.stats()
        assert after == stats
        again = ctx.cast_grid(cam, w, h)
        same(again, first)
        assert (ctx.stats()["last_kernel"], ctx.last_kernel_variant()) == kernel
    finally:
        dev.free()
        ctx.close()
