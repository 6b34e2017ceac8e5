"""Whole-tile pairs in trace_packet_rows_kernel<.., 2> (csrc/lane_map.h fast_launch / fast_grid: the short lane map, the straight-line
prologue and epilogue around the 128-ray walk): grids on the fast side of the rule and just off it, through mrt_cast(COHERENT) on
device rays (the width is found on the device) and mrt_cast_tiled, in both workgroup sizes.  Every cast record for record against the
oracle, and byte for byte against the same cast on a context whose tile order keeps it on the general map; both must have run the
same instantiation.  The camera looks at the soup's centre from outside and off every axis, so octants differ across the image and
the paired walk, the one-packet walk (pairs of two octants) and the generic walk (a packet of mixed octants) all run.  Which path a
launch took cannot be seen from here: tests/test_lane_map_fast_cpu.py holds the rule itself."""
import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
import parity

pytestmark = pytest.mark.gpu
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
N_TRIS = 2000
ORIGIN, FOV = (3.0, 2.2, -12.0), 70.0
FWD = tuple(-np.array(ORIGIN) / np.linalg.norm(ORIGIN))  # at the soup's centre (the origin)
FAST = [(32, 8), (16, 16), (48, 8), (64, 16)]  # 256 rays: the smallest batch whose width the device looks for; three pairs per tile row; two tile rows
OFF = [(24, 8), (16, 12), (40, 8)]             # an odd tile count; clipped rows; a width that is no multiple of 16
AWKWARD = [(48, 8), (64, 16)]                  # the fast grids that get awkward rays
GENERAL = dict(tile_order=3)                   # 32x32-tile super-tiles: none of these grids has them, so the order is row-major all the same


def _rays(w, h):
    rays = po.grid_rays(ORIGIN, FWD, w, h, FOV).copy()
    if (w, h) in AWKWARD:
        n = w * h
        rays["t_min"][3] = rays["t_max"][3]                          # degenerate: t_min == t_max
        rays["t_min"][n // 2 + 1] = 5.0; rays["t_max"][n // 2 + 1] = 1.0   # ... and t_min > t_max
        rays["direction"][7][0] = 0.0                                 # a zero direction component
        rays["direction"][n - 9][1] = 0.0
        rays["direction"][w + 2] = (0.0, 0.0, 1.0)                    # two of them
        rays["origin"][5] = (0.1, -0.2, 0.3)                       # origins inside the soup
        rays["origin"][n - 1] = (-1.5, 0.4, 2.0)
    return rays


@pytest.fixture(scope="module")
def soup(built):
    """a small soup with ids that differ from indices and three layers; rays and the oracle's records per grid, made once"""
    v = synth.soup(N_TRIS, 0.3, 11)
    ids = (5 * N_TRIS - 2 * np.arange(N_TRIS)).astype(np.uint32)
    layers = (1 << (np.arange(N_TRIS) % 3)).astype(np.uint32)
    osc = po.OracleScene(v, ids, layers)
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            rays = _rays(w, h)
            cache[(w, h)] = (rays, osc.trace(rays))
        return cache[(w, h)]
    return dict(v=v, ids=ids, layers=layers, get=get)


@pytest.fixture(scope="module", params=[64, 256], ids=["wg64", "wg256"])
def contexts(request, soup):
    """the context under test and its twin on the general map, same workgroup size"""
    pair = []
    for extra in ({}, GENERAL):
        c = capi.Context(0, kernel=capi.KERNEL_PACKET_DUAL, packet_wg=request.param, **extra)
        capi.Scene(soup["v"], soup["ids"], soup["layers"]).upload(c)
        pair.append(c)
    yield pair
    for c in pair:
        c.close()


def _cast(c, rays, w, h, tiled):
    n = w * h
    d_rays, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 32)
    got = np.zeros(n, dtype=T.HIT32)
    try:
        c.h2d(d_rays, rays)
        c.h2d(d_hits, np.full(n * 32, 0xA5, np.uint8))  # (a record no lane writes keeps a pattern no kernel writes)
        if tiled:
            c.cast_tiled(d_rays, d_hits, w, h)
        else:
            c.cast(d_rays, d_hits, count=n, flags=capi.FLAG_COHERENT | DEV)
        variant = c.last_kernel_variant()
        c.d2h(got, d_hits)
    finally:
        c.device_free(d_rays); c.device_free(d_hits)
    return got, variant


def _check(contexts, soup, w, h, tiled):
    rays, want = soup["get"](w, h)
    what = f"{w}x{h} {'mrt_cast_tiled' if tiled else 'mrt_cast(COHERENT)'}"
    got, variant = _cast(contexts[0], rays, w, h, tiled)
    assert variant.startswith("trace_packet_rows_kernel") and ", 2, " in variant, (what, variant)
    parity.assert_exact(got, want, what)
    twin, twin_variant = _cast(contexts[1], rays, w, h, tiled)
    assert variant == twin_variant, (what, variant, twin_variant)
    assert got.tobytes() == twin.tobytes(), f"{what}: differs from the general map's records"


@pytest.mark.parametrize("tiled", [False, True], ids=["cast", "tiled"])
@pytest.mark.parametrize("w,h", FAST + OFF, ids=lambda x: str(x))
def test_grids_on_the_fast_side_and_just_off_it(contexts, soup, w, h, tiled):
    rays, want = soup["get"](w, h)
    hit = want["prim_id"] >= 0
    assert hit.any() and (~hit).any()
    _check(contexts, soup, w, h, tiled)


def test_a_single_wave(contexts, soup):
    _check(contexts, soup, 16, 8, True)


def test_all_three_walk_forms_run(soup):
    """the rays of the largest fast grid: tile pairs of one octant (the paired walk), and a pair of one tile of mixed octants (the
    generic walk) beside a tile of one octant (the one-packet walk)"""
    rays, _ = soup["get"](64, 16)
    d = rays["direction"].reshape(16, 64, 3)
    forms = set()
    for ty in range(2):
        for pair in range(4):
            octs = []
            for t in range(2):
                flat = (d[ty * 8:ty * 8 + 8, (2 * pair + t) * 8:(2 * pair + t) * 8 + 8] < 0).reshape(-1, 3)
                octs.append(tuple(flat[0]) if (flat == flat[0]).all() else None)
            if None not in octs:
                forms.add("paired" if octs[0] == octs[1] else "two one-packet walks")
            elif octs != [None, None]:
                forms.add("generic and one-packet")
    assert {"paired", "generic and one-packet"} <= forms, forms


def test_format_neighbours_on_a_fast_shaped_grid(contexts, soup):
    """tokens, bools, 44-byte records and 60-byte rays on 64x16: the general map's formats, as today (oracle)"""
    w, h = 64, 16
    c = contexts[0]
    rays, want = soup["get"](w, h)
    n, hit = w * h, want["prim_id"] >= 0
    host = po.make_host_rays(rays)
    got44 = c.cast(host, flags=capi.FLAG_COHERENT | capi.FLAG_HOST_LAYOUT)
    assert c.last_kernel_variant().startswith("trace_packet_rows_kernel")
    assert got44.tobytes() == po.unpack_hits(want, host).tobytes(), "44-byte records from 60-byte rays"
    b = c.cast(rays, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_COHERENT | capi.FLAG_BOOL_OUT)
    assert np.array_equal(b, hit.astype(np.uint8)), "any-hit bools"
    d_rays, d_tok, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 4), c.device_alloc(n * 32)
    try:
        c.h2d(d_rays, rays)
        c.cast(d_rays, d_tok, count=n, flags=capi.FLAG_COHERENT | DEV | capi.FLAG_TOKEN_OUT)
        assert c.last_kernel_variant().startswith("trace_packet_rows_kernel")
        tok = np.zeros(n, np.uint32)
        c.d2h(tok, d_tok)
        assert np.array_equal(tok != capi.TOKEN_MISS, hit), "tokens"
        c.expand_tokens(d_rays, d_tok, d_hits, n)
        c.synchronize()
        rec = np.zeros(n, dtype=T.HIT32)
        c.d2h(rec, d_hits)
        parity.assert_exact(rec, want, "records rebuilt from the tokens")
    finally:
        c.device_free(d_rays); c.device_free(d_tok); c.device_free(d_hits)
    a = c.cast(rays, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_COHERENT)  # any hit, full records: the fast path's own store, SOME hit of the ray
    assert np.array_equal(a["prim_id"] >= 0, hit) and (a["t"][hit] >= want["t"][hit]).all(), "any-hit records"
    same = hit & (a["prim_id"] == want["prim_id"])
    assert a[same].tobytes() == want[same].tobytes(), "any-hit records of the closest triangle"
