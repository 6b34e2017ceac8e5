"""What one cast leaves for the next -- the width detect_grid_kernel found, tile schedules, the grid tuner's phase, the per-grid
state LRU -- across sequences of blocking, ASYNC, pipelined and submitted casts.  Every context here has MRT_POISON_OUTPUT set:
each cast first fills its output range with the byte 0xA5, which no kernel writes, so a record that no launch wrote cannot pass
for the previous frame's answer.  Caller-owned device buffers start out filled with the same pattern.  Every record of every
cast is compared with the oracle; bools and tokens against the oracle's prim_id."""
import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
import parity
import test_shadow_gpu as sh

pytestmark = pytest.mark.gpu
POISON = 0xA5
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
COH = capi.FLAG_COHERENT
ASYNC = capi.FLAG_ASYNC
CAM = ((0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0)
ASM, DUAL, AUTO = capi.KERNEL_PACKET_ASM, capi.KERNEL_PACKET_DUAL, capi.KERNEL_AUTO


class Soup:
    """a 20 000-triangle soup, its oracle, and the oracle's records of the grids and batches the tests cast (computed once)"""

    def __init__(self):
        self.verts = synth.soup(20000, 0.25, 41)
        self.scene, self.osc = capi.Scene(self.verts), po.OracleScene(self.verts)
        self._want = {}

    def view(self, w, h):
        if (w, h) not in self._want:
            rays = po.grid_rays(CAM[0], CAM[1], w, h, CAM[2])
            self._want[(w, h)] = (rays, self.osc.trace(rays, n_threads=16))
        return self._want[(w, h)]

    def incoherent(self, n):
        if n not in self._want:
            rays = synth.incoherent_rays(n, 17)
            self._want[n] = (rays, self.osc.trace(rays, n_threads=16))
        return self._want[n]


@pytest.fixture(scope="module")
def soup():
    return Soup()


def context(monkeypatch, kernel=AUTO, tile_schedule=0, min_log2=15):
    """a context with the output poison on; min_log2: MRT_SCHEDULE_MIN_LOG2 (0: the library's own bound)"""
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")
    if min_log2:
        monkeypatch.setenv("MRT_SCHEDULE_MIN_LOG2", str(min_log2))
    else:
        monkeypatch.delenv("MRT_SCHEDULE_MIN_LOG2", raising=False)
    return capi.Context(0, kernel=kernel, tile_schedule=tile_schedule)


class Bufs:
    """device buffers of one context, freed at the end"""

    def __init__(self, c):
        self.c, self.ptrs = c, []

    def put(self, arr):
        p = self.c.device_alloc(arr.nbytes)
        self.ptrs.append(p)
        self.c.h2d(p, arr)
        return p

    def poisoned(self, nbytes):
        return self.put(np.full(nbytes, POISON, dtype=np.uint8))

    def get(self, p, n, dtype=T.HIT32):
        out = np.zeros(n, dtype=dtype)
        self.c.d2h(out, p)
        return out

    def free(self):
        for p in self.ptrs:
            self.c.device_free(p)
        self.ptrs = []


def _where(idx, w, n):
    """which records (of a w-wide grid of n rays) and which 8x8 tiles they lie in"""
    ys, xs = idx // w, idx % w
    tiles = np.unique((ys // 8) * ((w + 7) // 8) + xs // 8)
    n_tiles = ((w + 7) // 8) * ((n // w + 7) // 8)
    return (f"{idx.size} of {n} records were never written, in {tiles.size} of {n_tiles} tiles "
            f"(tiles {tiles[0]}..{tiles[-1]}, rows {ys.min()}..{ys.max()})")


def check_hits(got, want, w, what):
    raw = got.view(np.uint8).reshape(got.shape[0], -1)
    idx = np.flatnonzero((raw == POISON).all(axis=1))
    assert idx.size == 0, f"{what}: " + _where(idx, w, got.shape[0])
    parity.assert_exact(got, want, what)


def check_bool(got, expect, w, what):
    idx = np.flatnonzero(got > 1)
    assert idx.size == 0, f"{what}: " + _where(idx, w, got.shape[0])
    assert np.array_equal(got.astype(bool), expect), what


def check_tokens(got, want, w, n_tris, what):
    idx = np.flatnonzero((got != capi.TOKEN_MISS) & (got >= n_tris))
    assert idx.size == 0, f"{what}: " + _where(idx, w, got.shape[0])
    assert np.array_equal(got != capi.TOKEN_MISS, want["prim_id"] >= 0), what


# The scheduled launches: the explicit packet kernels with the schedule's bound at 2^15 rays (pieces, no pieces, no schedule),
# and MRT_KERNEL_AUTO at sizes it schedules by default.
def _sched_params(auto_wh):
    ps = [pytest.param(k, ts, 15, wh, id=f"{name}-schedule{ts}") for k, name, wh in ((ASM, "asm", (256, 128)), (DUAL, "dual", (256, 128)))
          for ts in (0, 2, 1)]
    return ps + [pytest.param(AUTO, 0, 0, auto_wh, id="auto")]


@pytest.mark.parametrize("kernel,tile_schedule,min_log2,a_wh", _sched_params((640, 360)))
def test_stale_width_async(built, soup, monkeypatch, kernel, tile_schedule, min_log2, a_wh):
    """A grid A is cast (blocking, COHERENT, its width found on the device) until its schedule has an order; then, behind a long
    ASYNC incoherent cast, two ASYNC COHERENT casts B1, B2 of a larger grid with as many rays as each other.  When B2 is queued,
    B1's detect has not run: a plan made from B1's count and the words the device has written so far would schedule B2 from A's
    width, and launch too few lanes for B's tiles (plans: csrc/host/launch_policy_test.cpp, memo)."""
    (aw, ah), (bw, bh) = a_wh, (1280, 960)
    c = context(monkeypatch, kernel, tile_schedule, min_log2)
    soup.scene.upload(c)
    ra, wa = soup.view(aw, ah)
    rb, wb = soup.view(bw, bh)
    inc, wi = soup.incoherent(1 << 21)
    na, nb, ni = ra.shape[0], rb.shape[0], inc.shape[0]
    d = Bufs(c)
    try:
        da, db, di = d.put(ra), d.put(rb), d.put(inc)
        out_a, out_i = d.poisoned(na * 32), d.poisoned(ni * 32)
        outs = [d.poisoned(nb * 32) for _ in range(4)]
        for f in range(3):
            c.cast(da, out_a, count=na, flags=DEV | COH)
            check_hits(d.get(out_a, na), wa, aw, f"A {aw}x{ah} frame {f}")
        c.cast(di, out_i, count=ni, flags=DEV | ASYNC)             # milliseconds of work in front of B1 and B2
        c.cast(db, outs[0], count=nb, flags=DEV | COH | ASYNC)     # B1
        c.cast(db, outs[1], count=nb, flags=DEV | COH | ASYNC)     # B2: as many rays as B1
        c.synchronize()
        parity.assert_exact(d.get(out_i, ni), wi, "the ASYNC incoherent cast in front")
        check_hits(d.get(outs[0], nb), wb, bw, "ASYNC B1")
        check_hits(d.get(outs[1], nb), wb, bw, "ASYNC B2 (the count of B1, the width of A?)")
        c.cast(db, outs[2], count=nb, flags=DEV | COH)             # blocking: from B's own width
        check_hits(d.get(outs[2], nb), wb, bw, "blocking B3")
        c.cast(db, outs[3], count=nb, flags=DEV | COH | ASYNC)
        c.synchronize()
        check_hits(d.get(outs[3], nb), wb, bw, "ASYNC B4")
        c.cast(da, out_a, count=na, flags=DEV | COH)
        check_hits(d.get(out_a, na), wa, aw, "A after B")
    finally:
        d.free()
        c.close()


@pytest.mark.parametrize("kernel,min_log2", [pytest.param(ASM, 15, id="asm"), pytest.param(DUAL, 15, id="dual"), pytest.param(AUTO, 0, id="auto")])
def test_stale_width_pipelined(built, soup, monkeypatch, kernel, min_log2):
    """Blocking 1024x576 casts from host arrays, then a host cast of 2048x1152 rays: the upload / trace / download pipeline in
    2^20-ray chunks (2048 x 512, 2048 x 512, 2048 x 128), each queued behind the one before without a wait."""
    c = context(monkeypatch, kernel, 0, min_log2)
    soup.scene.upload(c)
    ra, wa = soup.view(1024, 576)
    rb, wb = soup.view(2048, 1152)
    try:
        for f in range(3):
            check_hits(c.cast(ra, flags=COH), wa, 1024, f"1024x576 frame {f}")
        for f in range(2):
            check_hits(c.cast(rb, flags=COH), wb, 2048, f"pipelined 2048x1152 cast {f}")
        check_hits(c.cast(ra, flags=COH), wa, 1024, "1024x576 after the pipeline")
        check_bool(c.cast(rb, mode=capi.MODE_ANY_HIT, flags=COH | capi.FLAG_BOOL_OUT), wb["prim_id"] >= 0, 2048, "pipelined any-hit")
    finally:
        c.close()


@pytest.mark.parametrize("kernel,tile_schedule,min_log2,wh", [
    pytest.param(ASM, 0, 15, (512, 256), id="asm-schedule0"), pytest.param(ASM, 2, 15, (512, 256), id="asm-schedule2"),
    pytest.param(DUAL, 0, 15, (512, 256), id="dual-schedule0"), pytest.param(DUAL, 2, 15, (512, 256), id="dual-schedule2"),
    pytest.param(AUTO, 0, 0, (1024, 576), id="auto")])
def test_async_frame_loop(built, soup, monkeypatch, kernel, tile_schedule, min_log2, wh):
    """One scheduled grid: four blocking frames (the grid tuner's timed phases under MRT_KERNEL_AUTO), then twelve ASYNC frames
    into separate buffers -- mrt_cast_grid and mrt_cast(COHERENT) of the same rays in turn, no host wait between them: the
    schedule's two generations and the tuner's ASYNC frames --, one synchronize, then a blocking frame; three rounds."""
    w, h = wh
    c = context(monkeypatch, kernel, tile_schedule, min_log2)
    soup.scene.upload(c)
    rays, want = soup.view(w, h)
    n = rays.shape[0]
    cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
    d = Bufs(c)
    try:
        d_rays = d.put(rays)
        outs = [d.poisoned(n * 32) for _ in range(12)]
        for rnd in range(3):
            for f in range(4):
                c.cast_grid(cam, w, h, hits=outs[0], flags=capi.FLAG_HITS_ON_DEVICE)
                check_hits(d.get(outs[0], n), want, w, f"round {rnd} blocking frame {f} ({c.last_kernel_variant()})")
            for k in range(12):
                if k % 2:
                    c.cast(d_rays, outs[k], count=n, flags=DEV | COH | ASYNC)
                else:
                    c.cast_grid(cam, w, h, hits=outs[k], flags=capi.FLAG_HITS_ON_DEVICE | ASYNC)
            c.synchronize()
            for k in range(12):
                check_hits(d.get(outs[k], n), want, w, f"round {rnd} ASYNC frame {k} ({'mrt_cast' if k % 2 else 'mrt_cast_grid'})")
            c.cast(d_rays, outs[0], count=n, flags=DEV | COH)
            check_hits(d.get(outs[0], n), want, w, f"round {rnd} blocking mrt_cast after the loop")
    finally:
        d.free()
        c.close()


@pytest.mark.parametrize("kernel", [ASM, DUAL])
def test_lru_eviction_rebuilds_states(built, soup, monkeypatch, kernel):
    """Ten grid and mode keys (five row blocks of one grid, nearest and any-hit) cast in turn for three rounds: the per-grid state
    LRU holds eight (GridStates::kCount), so every round evicts and rebuilds states and their tile schedules."""
    c = context(monkeypatch, kernel, 0, 15)
    soup.scene.upload(c)
    w, h = 512, 256
    rays, want = soup.view(w, h)
    cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
    blocks = [(0, 64), (64, 128), (128, 192), (192, 256), (0, 128)]     # 2^15 rays and more each: all scheduled
    try:
        for rnd in range(3):
            for (y0, y1) in blocks:
                sel = want[y0 * w:y1 * w]
                check_hits(c.cast_grid(cam, w, h, y0=y0, y1=y1), sel, w, f"round {rnd} rows [{y0}, {y1})")
                b = c.cast_grid(cam, w, h, y0=y0, y1=y1, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
                check_bool(b, sel["prim_id"] >= 0, w, f"round {rnd} rows [{y0}, {y1}) any-hit")
    finally:
        c.close()


@pytest.mark.parametrize("kernel,min_log2", [pytest.param(ASM, 15, id="asm"), pytest.param(DUAL, 15, id="dual"), pytest.param(AUTO, 0, id="auto")])
def test_state_kept_across_refit_and_shadows(built, monkeypatch, kernel, min_log2):
    """A schedule is learnt (grid casts and mrt_cast(COHERENT) of the same rays), then the triangles move (mrt_refit_scene) and
    shadow casts run between the frames: the next scheduled frames are the new scene's records, the shadow masks the new
    scene's."""
    c = context(monkeypatch, kernel, 0, min_log2)
    v = synth.soup(20000, 0.25, 9)
    nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(v))
    c.upload_scene(capi.make_triangles(v), nodes, prim_idx)
    w, h = (512, 256) if kernel != AUTO else (640, 360)
    rays = po.grid_rays(CAM[0], CAM[1], w, h, CAM[2])
    n = rays.shape[0]
    cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
    lights = np.concatenate([sh.light(T.LIGHT_DIRECTIONAL, direction=(0.2, 0.3, -1.0)), sh.light(T.LIGHT_POINT, pos=(1.0, 0.5, -9.0))])
    d = Bufs(c)
    try:
        d_rays = d.put(rays)
        d_grid, d_cast = d.poisoned(n * 32), d.poisoned(n * 32)
        d_mask = d.poisoned(n * len(lights))
        want = po.OracleScene(v).trace(rays, n_threads=16)
        for f in range(4):
            c.cast_grid(cam, w, h, hits=d_grid, flags=capi.FLAG_HITS_ON_DEVICE)
            check_hits(d.get(d_grid, n), want, w, f"frame {f} before the refit")
            c.cast(d_rays, d_cast, count=n, flags=DEV | COH)
            check_hits(d.get(d_cast, n), want, w, f"mrt_cast frame {f} before the refit")
        for k in range(3):
            v1 = synth.deform(v, 0.05 * (k + 1), 1.3, 3)
            c.refit_scene(capi.make_triangles(v1))
            osc = po.OracleScene(v1)
            want = osc.trace(rays, n_threads=16)
            hit = want["prim_id"] >= 0
            with np.errstate(over="ignore", invalid="ignore"):  # (the position of a miss is not used)
                pos = rays["origin"] + rays["direction"] * want["t"][:, None]
            srays, traced = sh.shadow_rays(pos, want["normal"], hit, lights)
            lit = (~(traced & (osc.trace(srays, any_hit=True, n_threads=16)["prim_id"] >= 0))).astype(np.uint8)
            for f in range(2):
                c.cast_grid(cam, w, h, hits=d_grid, flags=capi.FLAG_HITS_ON_DEVICE)
                check_hits(d.get(d_grid, n), want, w, f"refit {k} frame {f}")
                c.cast_grid_shadows(cam, w, h, d_grid, lights, d_mask)
                check_bool(d.get(d_mask, n * len(lights), np.uint8), lit == 1, w, f"refit {k} grid shadows {f}")
                c.cast(d_rays, d_cast, count=n, flags=DEV | COH)
                check_hits(d.get(d_cast, n), want, w, f"refit {k} mrt_cast frame {f}")
                c.cast_shadows(d_rays, d_cast, n, lights, d_mask, flags=ASYNC)
                c.synchronize()
                check_bool(d.get(d_mask, n * len(lights), np.uint8), lit == 1, w, f"refit {k} shadows {f}")
    finally:
        d.free()
        c.close()


@pytest.mark.parametrize("kernel,min_log2", [pytest.param(ASM, 15, id="asm"), pytest.param(DUAL, 15, id="dual"), pytest.param(AUTO, 0, id="auto")])
def test_submit_collect_between_other_casts(built, soup, monkeypatch, kernel, min_log2):
    """mrt_submit / mrt_collect of one batch, interleaved with blocking casts of other sizes, grid casts and small host casts
    (the mapped-memory path): records, tokens and bools of every one."""
    c = context(monkeypatch, kernel, 0, min_log2)
    soup.scene.upload(c)
    ra, wa = soup.view(640, 360)
    rb, wb = soup.view(512, 256)
    rg, wg = soup.view(400, 304)
    cam_g = capi.camera_look(CAM[0], CAM[1], 400, 304, CAM[2])
    n_tris = soup.verts.shape[0]
    try:
        for rnd in range(4):
            c.submit(ra, flags=COH)
            check_hits(c.collect(), wa, 640, f"round {rnd} collected")
            check_hits(c.cast(rb, flags=COH), wb, 512, f"round {rnd} blocking 512x256")
            c.submit(rb, flags=COH | capi.FLAG_TOKEN_OUT)
            check_tokens(c.collect(), wb, 512, n_tris, f"round {rnd} collected tokens")
            check_hits(c.cast_grid(cam_g, 400, 304), wg, 400, f"round {rnd} grid 400x304")
            check_hits(c.cast(ra[:1000], flags=COH), wa[:1000], 640, f"round {rnd} small host cast")
            c.submit(ra, mode=capi.MODE_ANY_HIT, flags=COH | capi.FLAG_BOOL_OUT)
            check_bool(c.collect(), wa["prim_id"] >= 0, 640, f"round {rnd} collected any-hit")
            check_hits(c.cast(ra, flags=COH), wa, 640, f"round {rnd} blocking 640x360")
    finally:
        c.close()
