"""The row kernels' prologue and epilogue (trace_packet_rows_kernel: one tile map per wave, csrc/lane_map.h; the record made from the
winning triangle's own row) on every edge of the map: unpaired tiles, clipped grids, every tile order, width and workgroup size,
culling on and off, every entry and output format, a query mask, linear batches around a wave, the scheduled size cast until the
measured order and the pieces are in use, and a refit.  Every field of every record against the oracle; every cast forces
MRT_KERNEL_PACKET_ROWS or MRT_KERNEL_PACKET_DUAL and checks that a row kernel ran."""
import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
import parity

pytestmark = pytest.mark.gpu
ROWS, DUAL = capi.KERNEL_PACKET_ROWS, capi.KERNEL_PACKET_DUAL
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
ORIGIN, FWD, FOV = (0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0
N_TRIS = 2000
GRIDS = [(8, 8), (16, 8), (24, 8), (17, 9), (130, 66)]  # one unpaired tile; a pair; a pair plus a single; clipped right and bottom


@pytest.fixture(scope="module")
def soup(built):
    """2 000 triangles whose ids differ from their indices, in three layers; the oracle's records per grid, traced once"""
    v = synth.soup(N_TRIS, 0.4, 3)
    ids = (7 * N_TRIS - 3 * np.arange(N_TRIS)).astype(np.uint32)
    layers = (1 << (np.arange(N_TRIS) % 3)).astype(np.uint32)
    osc = po.OracleScene(v, ids, layers)
    cache = {}

    def want(w, h, mask=0xFFFFFFFF):
        if (w, h, mask) not in cache:
            cache[(w, h, mask)] = osc.trace(rays(w, h), query_mask=mask)
        return cache[(w, h, mask)]

    def rays(w, h):
        if (w, h) not in cache:
            cache[(w, h)] = po.grid_rays(ORIGIN, FWD, w, h, FOV)
        return cache[(w, h)]
    return dict(v=v, ids=ids, layers=layers, osc=osc, want=want, rays=rays)


def _context(soup, **opts):
    c = capi.Context(0, **opts)
    capi.Scene(soup["v"], soup["ids"], soup["layers"]).upload(c)
    return c


def _ran_rows(c, what):
    assert c.last_kernel_variant().startswith("trace_packet_rows_kernel"), (what, c.last_kernel_variant())


def _every_entry(c, soup, w, h, what, mask=0xFFFFFFFF):
    """mrt_cast(COHERENT) on device rays, mrt_cast_grid, mrt_cast_tiled: closest hit, 32-byte records"""
    n, rays, want = w * h, soup["rays"](w, h), soup["want"](w, h, mask)
    cam = capi.camera_look(ORIGIN, FWD, w, h, FOV)
    d_rays, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 32)
    got = np.zeros(n, dtype=T.HIT32)
    try:
        c.h2d(d_rays, rays)
        c.cast(d_rays, d_hits, count=n, query_mask=mask, flags=capi.FLAG_COHERENT | DEV)
        _ran_rows(c, what + " cast")
        c.d2h(got, d_hits)
        parity.assert_exact(got, want, f"{what}: mrt_cast(COHERENT) on device rays")
        parity.assert_exact(c.cast_grid(cam, w, h, query_mask=mask), want, f"{what}: mrt_cast_grid")
        _ran_rows(c, what + " cast_grid")
        c.h2d(d_hits, np.zeros(n, dtype=T.HIT32))
        c.cast_tiled(d_rays, d_hits, w, h, query_mask=mask)
        _ran_rows(c, what + " cast_tiled")
        c.d2h(got, d_hits)
        parity.assert_exact(got, want, f"{what}: mrt_cast_tiled")
    finally:
        c.device_free(d_rays); c.device_free(d_hits)


def _every_format(c, soup, w, h, what, mask=0xFFFFFFFF):
    """any hit; 44-byte records from 60-byte rays, tokens (expanded to records), bools"""
    n, rays, want = w * h, soup["rays"](w, h), soup["want"](w, h, mask)
    hit = want["prim_id"] >= 0
    cam = capi.camera_look(ORIGIN, FWD, w, h, FOV)
    host = po.make_host_rays(rays)
    got44 = c.cast(host, query_mask=mask, flags=capi.FLAG_COHERENT | capi.FLAG_HOST_LAYOUT)
    _ran_rows(c, what + " 44-byte records")
    assert got44.tobytes() == po.unpack_hits(want, host).tobytes(), f"{what}: 44-byte records"
    tok = c.cast_grid(cam, w, h, query_mask=mask, flags=capi.FLAG_TOKEN_OUT)
    _ran_rows(c, what + " tokens")
    assert np.array_equal(tok != capi.TOKEN_MISS, hit), f"{what}: tokens"
    d_rays, d_tok, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 4), c.device_alloc(n * 32)
    try:
        c.h2d(d_rays, rays); c.h2d(d_tok, tok)
        c.expand_tokens(d_rays, d_tok, d_hits, n)
        c.synchronize()
        rec = np.zeros(n, dtype=T.HIT32)
        c.d2h(rec, d_hits)
        parity.assert_exact(rec, want, f"{what}: records rebuilt from the tokens")
    finally:
        c.device_free(d_rays); c.device_free(d_tok); c.device_free(d_hits)
    b = c.cast_grid(cam, w, h, query_mask=mask, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
    _ran_rows(c, what + " any-hit bools")
    assert np.array_equal(b, hit.astype(np.uint8)), f"{what}: any-hit bools"
    b = c.cast(rays, query_mask=mask, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_COHERENT | capi.FLAG_BOOL_OUT)
    assert np.array_equal(b, hit.astype(np.uint8)), f"{what}: any-hit bools of rays from memory"
    a = c.cast(rays, query_mask=mask, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_COHERENT)  # any hit, full records: SOME hit of the ray
    _ran_rows(c, what + " any-hit records")
    assert np.array_equal(a["prim_id"] >= 0, hit) and (a["t"][hit] >= want["t"][hit]).all(), f"{what}: any-hit records"
    same = hit & (a["prim_id"] == want["prim_id"])
    assert a[same].tobytes() == want[same].tobytes(), f"{what}: any-hit records of the closest triangle"
    by_id = {int(i): int(l) for i, l in zip(soup["ids"], soup["layers"])}
    assert all(by_id[int(p)] == int(l) for p, l in zip(a["prim_id"][hit], a["hit_layers"][hit])), f"{what}: any-hit layers go with the id"


@pytest.mark.parametrize("kernel", [ROWS, DUAL], ids=["rows", "dual"])
@pytest.mark.parametrize("w,h", GRIDS)
def test_grids_with_unpaired_and_clipped_tiles(soup, kernel, w, h):
    c = _context(soup, kernel=kernel)
    try:
        _every_entry(c, soup, w, h, f"{w}x{h}")
        _every_format(c, soup, w, h, f"{w}x{h}")
        _every_entry(c, soup, w, h, f"{w}x{h} without layer 2", mask=0x5)   # a query mask that excludes one layer
        _every_format(c, soup, w, h, f"{w}x{h} without layer 2", mask=0x5)
    finally:
        c.close()


@pytest.mark.parametrize("opts,w,h", [
    (dict(tile_order=1), 128, 128), (dict(tile_order=2), 256, 256), (dict(tile_order=3), 512, 64),
    (dict(tile_w_log2=2), 130, 66), (dict(tile_w_log2=4), 130, 66), (dict(xcd_swizzle=1), 130, 66),
    (dict(packet_wg=64), 130, 66), (dict(packet_wg=256), 130, 66), (dict(packet_wg=256), 24, 8),
    (dict(packet_cull=1), 130, 66), (dict(packet_cull=2), 130, 66), (dict(packet_cull=2), 17, 9)],
    ids=lambda x: "_".join(f"{k}{v}" for k, v in x.items()) if isinstance(x, dict) else str(x))
@pytest.mark.parametrize("kernel", [ROWS, DUAL], ids=["rows", "dual"])
def test_tile_orders_widths_workgroups_and_culling(soup, kernel, opts, w, h):
    c = _context(soup, kernel=kernel, **opts)
    try:
        _every_entry(c, soup, w, h, f"{opts} {w}x{h}")
        b = c.cast_grid(capi.camera_look(ORIGIN, FWD, w, h, FOV), w, h, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        assert np.array_equal(b, (soup["want"](w, h)["prim_id"] >= 0).astype(np.uint8)), f"{opts}: any hit"
    finally:
        c.close()


@pytest.mark.parametrize("kernel", [ROWS, DUAL], ids=["rows", "dual"])
def test_linear_batches_around_a_wave(soup, kernel):
    """1, 63, 65 and 129 rays declared coherent (no grid to find: the linear map), from host and from device memory"""
    c = _context(soup, kernel=kernel)
    try:
        rays = soup["rays"](130, 66)[130 * 30 + 7:]
        for n in (1, 63, 65, 129):
            want = soup["osc"].trace(rays[:n])
            parity.assert_exact(c.cast(rays[:n], flags=capi.FLAG_COHERENT), want, f"{n} rays")
            _ran_rows(c, f"{n} rays")
            d_rays, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 32)
            c.h2d(d_rays, np.ascontiguousarray(rays[:n]))
            c.cast(d_rays, d_hits, count=n, flags=capi.FLAG_COHERENT | DEV)
            got = np.zeros(n, dtype=T.HIT32)
            c.d2h(got, d_hits)
            c.device_free(d_rays); c.device_free(d_hits)
            parity.assert_exact(got, want, f"{n} rays on the device")
            b = c.cast(rays[:n], mode=capi.MODE_ANY_HIT, flags=capi.FLAG_COHERENT | capi.FLAG_BOOL_OUT)
            assert np.array_equal(b, (want["prim_id"] >= 0).astype(np.uint8)), f"{n} rays, any hit"
    finally:
        c.close()


@pytest.mark.parametrize("kernel", [ROWS, DUAL], ids=["rows", "dual"])
def test_scheduled_grid_cast_fourteen_times(soup, kernel, monkeypatch):
    """512x256 = 2^17 rays, the smallest grid that is scheduled: by the fourteenth cast the measured order and the pieces are in use"""
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")   # every output starts as a pattern no kernel writes: a skipped tile shows
    w, h = 512, 256
    n, rays, want = w * h, soup["rays"](w, h), soup["want"](w, h)
    cam = capi.camera_look(ORIGIN, FWD, w, h, FOV)
    c = _context(soup, kernel=kernel)
    d_rays, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 32)
    got = np.zeros(n, dtype=T.HIT32)
    try:
        c.h2d(d_rays, rays)
        for frame in range(14):
            c.cast(d_rays, d_hits, count=n, flags=capi.FLAG_COHERENT | DEV)
            _ran_rows(c, f"frame {frame}")
            c.d2h(got, d_hits)
            parity.assert_exact(got, want, f"mrt_cast(COHERENT) frame {frame}")
            parity.assert_exact(c.cast_grid(cam, w, h), want, f"mrt_cast_grid frame {frame}")
            c.cast_tiled(d_rays, d_hits, w, h)
            c.d2h(got, d_hits)
            parity.assert_exact(got, want, f"mrt_cast_tiled frame {frame}")
        tok = c.cast_grid(cam, w, h, flags=capi.FLAG_TOKEN_OUT)
        assert np.array_equal(tok != capi.TOKEN_MISS, want["prim_id"] >= 0)
        b = c.cast_grid(cam, w, h, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        assert np.array_equal(b, (want["prim_id"] >= 0).astype(np.uint8))
    finally:
        c.device_free(d_rays); c.device_free(d_hits)
        c.close()


@pytest.mark.parametrize("kernel", [ROWS, DUAL], ids=["rows", "dual"])
def test_records_after_a_refit_come_from_the_new_rows(soup, kernel):
    """mrt_refit_scene with moved vertices, new ids and new layers: normals, ids and layers of every record are the oracle's of the new
    triangles (the record is made from the triangle's row, which the refit rewrites)"""
    v = soup["v"]
    v1 = synth.deform(v, 0.12, 0.7, 3)
    ids1 = (N_TRIS + 5 + np.arange(N_TRIS)[::-1]).astype(np.uint32)
    layers1 = (1 << ((np.arange(N_TRIS) + 1) % 3)).astype(np.uint32)
    osc1 = po.OracleScene(v1, ids1, layers1)
    w, h = 130, 66
    rays = soup["rays"](w, h)
    cam = capi.camera_look(ORIGIN, FWD, w, h, FOV)
    c = _context(soup, kernel=kernel)
    try:
        parity.assert_exact(c.cast_grid(cam, w, h), soup["want"](w, h), "before the refit")
        c.refit_scene(capi.make_triangles(v1, ids1, layers1))
        for mask in (0xFFFFFFFF, 0x6):
            want = osc1.trace(rays, query_mask=mask)
            assert (want["prim_id"] >= 0).any()
            parity.assert_exact(c.cast_grid(cam, w, h, query_mask=mask), want, f"after the refit, mask {mask:#x}: mrt_cast_grid")
            _ran_rows(c, "after the refit")
            parity.assert_exact(c.cast(rays, query_mask=mask, flags=capi.FLAG_COHERENT), want, f"after the refit, mask {mask:#x}: mrt_cast")
            host = po.make_host_rays(rays)
            got44 = c.cast(host, query_mask=mask, flags=capi.FLAG_COHERENT | capi.FLAG_HOST_LAYOUT)
            assert got44.tobytes() == po.unpack_hits(want, host).tobytes(), "after the refit: 44-byte records"
    finally:
        c.close()
