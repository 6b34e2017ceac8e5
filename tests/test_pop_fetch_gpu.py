"""The pop of the row walks (csrc/packet_rows_kernel.h): in builds with -DMRT_ROWS_POPFETCH=1 the popped row's fetch is issued from a
scalar shadow of the top entry's ref before the entry is read from the LDS, and the entry BELOW the popped one is read for the new
shadow; the default build reads the entry first (DESIGN 4.1b round 6 says why).  These tests hold either build (MRT_LIB_PATH names
the library).  What can go wrong is a pop pattern, so the scenes here are the smallest that force each one, a wave or a few per
cast, on every form that has a pop:

  behind    two triangles behind the camera: the first pop finds the sentinel (no entry below it may be read);
  chain(2)  deep_tree's chain of two leaves: one push, one pop, then the sentinel (the stack at depth 1);
  chain(63), chain(64)   the stack at its bound and one below: ray j's answer comes out of entry j, the bottom two included;
  soup      2 000 triangles: pop -> dead-end node -> pop -> leaf -> pop, the reloaded shadow used at once (the counting build must
            report a high-water mark of 3 or more, or the scene does not do that).

Forms: the paired walk on the whole-tile fast path (width a multiple of 16, rows of 8) and on the general code (the same grids under
a tile order the fast rule refuses, and widths 40 and 72), in 64- and 256-thread workgroups; the one-packet loop (the odd tile of
those widths, a pair split by the octant change at the image centre, and MRT_KERNEL_PACKET_ROWS); the culling loop through
mrt_cast_grid; any hit, which leaves the walk with entries on the stack; the counting builds.  Every record bit for bit against the
oracle (the chains: against the brute-force test of every triangle, which the oracle's walk equals there: test_deep_trees_cpu.py)."""
import numpy as np
import pytest

import deep_tree as dt
from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
import parity

pytestmark = pytest.mark.gpu
ROWS, DUAL = capi.KERNEL_PACKET_ROWS, capi.KERNEL_PACKET_DUAL
ORIGIN, FWD, FOV = (0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0   # along +z: dx and dy change sign at the image centre
N_TRIS = 2000
# Two tile rows each, so that no tile straddles the sign change of dy (a tile of mixed octants takes the generic C++ walk, which has no
# such pop).  32 and 64 wide: every pair of one octant; 48: the middle pair of each tile row is split by the sign change of dx (two
# one-packet walks).  40 and 72 wide (widths fast_grid refuses, an odd tile count): the middle tile is of mixed octants, its partner
# and the last tile of the row take the one-packet loop, the other pairs the paired walk of the general code.
FAST_GRIDS = [(32, 16), (64, 16), (48, 16)]
OFF_GRIDS = [(40, 16), (72, 16)]

# form -> (context options, how the rays get there, the instantiation's template arguments after <any hit, counting,)
FORMS = {
    "pair_fast_wg64": (dict(kernel=DUAL, packet_wg=64, packet_cull=1), "tiled", "2, 64, false>"),
    "pair_fast_wg256": (dict(kernel=DUAL, packet_wg=256, packet_cull=1), "tiled", "2, 256, false>"),
    "pair_general_wg64": (dict(kernel=DUAL, packet_wg=64, packet_cull=1, tile_order=3), "tiled", "2, 64, false>"),   # (no 32x32 super-tiles here: row-major all the same)
    "pair_general_wg256": (dict(kernel=DUAL, packet_wg=256, packet_cull=1, tile_order=3), "tiled", "2, 256, false>"),
    "cull_wg64": (dict(kernel=DUAL, packet_wg=64, packet_cull=2), "grid", "2, 64, true>"),
    "cull_wg256": (dict(kernel=DUAL, packet_wg=256, packet_cull=2), "grid", "2, 256, true>"),
    "one_packet": (dict(kernel=ROWS), "tiled", "1, 256, false>"),
}
SCENES = ["behind", "chain2", "chain63", "chain64", "soup"]


class Scene:
    """a scene, its rays per grid (from memory: `mem`; of the camera: `cam`) and the expected records, made once and never changed"""

    def __init__(self, name):
        self.name, self.cache = name, {}
        if name.startswith("chain"):
            self.n = int(name[5:])
            self.s = dt.prepared(self.n)
            self.camera = dt.grid_camera(self.n)
        else:
            if name == "behind":   # two triangles behind the camera: every ray misses the root's children
                v = np.float32([[[-1, -1, -20], [1, -1, -20], [0, 1, -20]], [[-1, -1, -24], [1, -1, -24], [0, 1, -24]]])
                ids, layers = np.uint32([7, 3]), np.uint32([1, 2])
            else:
                v = synth.soup(N_TRIS, 0.4, 3)
                ids = (7 * N_TRIS - 3 * np.arange(N_TRIS)).astype(np.uint32)
                layers = (1 << (np.arange(N_TRIS) % 3)).astype(np.uint32)
            self.v, self.ids, self.layers = v, ids, layers
            self.osc = po.OracleScene(v, ids, layers)
            # (behind: a camera off every axis, so narrow that all its rays share one octant and a single wave, 16x8, takes the paired walk)
            self.camera = (ORIGIN, (3.0 ** -0.5,) * 3, 30.0) if name == "behind" else (ORIGIN, FWD, FOV)

    def upload(self, c):
        if self.name.startswith("chain"):
            c.upload_scene(self.s["tris"], self.s["nodes"], self.s["prim_idx"])
            assert c.scene_info()["stack_need"] == self.n
        else:
            capi.Scene(self.v, self.ids, self.layers).upload(c)

    def _trace(self, rays, any_hit=False):
        if self.name.startswith("chain"):
            return po.trace_brute(self.s["tris"], rays, any_hit=any_hit)
        return self.osc.trace(rays, any_hit=any_hit)

    def rays(self, how, w, h):
        """(rays, expected records).  Chains from memory: the forward rays in turn (one octant, every tile holds every depth)."""
        key = (how, w, h)
        if key not in self.cache:
            if how == "mem" and self.name.startswith("chain"):
                rays = np.ascontiguousarray(dt.forward_rays(self.n, w * h))
            else:
                rays = po.grid_rays(*self.camera[:2], w, h, self.camera[2])
            self.cache[key] = (rays, self._trace(rays))
        return self.cache[key]


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = Scene(name)
    return _SCENES[name]


def _tiled(c, rays, w, h, mode=capi.MODE_NEAREST):
    n = w * h
    d_rays, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 32)
    got = np.zeros(n, dtype=T.HIT32)
    try:
        c.h2d(d_rays, rays)
        c.h2d(d_hits, np.full(n * 32, 0xA5, np.uint8))   # a record no lane writes keeps a pattern no kernel writes
        c.cast_tiled(d_rays, d_hits, w, h, mode=mode)
        variant = c.last_kernel_variant()
        c.d2h(got, d_hits)
    finally:
        c.device_free(d_rays); c.device_free(d_hits)
    return got, variant


def _check_any(a, want, what):
    """any-hit records: SOME hit of every ray that has one; the closest triangle's record where that is the one found"""
    hit = want["prim_id"] >= 0
    assert np.array_equal(a["prim_id"] >= 0, hit) and (a["t"][hit] >= want["t"][hit]).all(), f"{what}: any-hit records"
    same = hit & (a["prim_id"] == want["prim_id"])
    assert a[same].tobytes() == want[same].tobytes(), f"{what}: any-hit records of the closest triangle"


def _cast_form(c, sc, how, tail, w, h):
    what = f"{sc.name} {w}x{h} {tail}"
    if how == "tiled":
        rays, want = sc.rays("mem", w, h)
        got, variant = _tiled(c, rays, w, h)
        assert variant == "trace_packet_rows_kernel<false, false, " + tail, (what, variant)
        parity.assert_exact(got, want, what)
        a, variant = _tiled(c, rays, w, h, mode=capi.MODE_ANY_HIT)   # ends with entries left on the stack
        assert variant == "trace_packet_rows_kernel<true, false, " + tail, (what, variant)
        _check_any(a, want, what)
        got, _ = _tiled(c, rays, w, h)                               # ... and the next walk starts from an empty one
        parity.assert_exact(got, want, what + " after the any-hit cast")
        if w * h >= 256:   # mrt_cast(COHERENT) on device rays: the width is found on the device
            n = w * h
            d_rays, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 32)
            try:
                c.h2d(d_rays, rays)
                c.cast(d_rays, d_hits, count=n, flags=capi.FLAG_COHERENT | capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE)
                assert c.last_kernel_variant().startswith("trace_packet_rows_kernel<false, false, "), (what, c.last_kernel_variant())
                got = np.zeros(n, dtype=T.HIT32)
                c.d2h(got, d_hits)
            finally:
                c.device_free(d_rays); c.device_free(d_hits)
            parity.assert_exact(got, want, what + " mrt_cast(COHERENT)")
    else:
        rays, want = sc.rays("cam", w, h)
        cam = capi.camera_look(*sc.camera[:2], w, h, sc.camera[2])
        got = c.cast_grid(cam, w, h)
        assert c.last_kernel_variant() == "trace_packet_rows_kernel<false, false, " + tail, (what, c.last_kernel_variant())
        parity.assert_exact(got, want, what)
        lit = c.cast_grid(cam, w, h, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        assert c.last_kernel_variant() == "trace_packet_rows_kernel<true, false, " + tail, (what, c.last_kernel_variant())
        assert np.array_equal(lit.astype(bool), want["prim_id"] >= 0), f"{what}: any-hit bools"
        parity.assert_exact(c.cast_grid(cam, w, h), want, what + " after the any-hit cast")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SCENES)
def test_every_pop_pattern_on_every_form(built, name, form):
    opts, how, tail = FORMS[form]
    sc = scene(name)
    c = capi.Context(0, **opts)
    try:
        sc.upload(c)
        for w, h in FAST_GRIDS + OFF_GRIDS + ([(16, 8)] if name == "behind" else []):
            _cast_form(c, sc, how, tail, w, h)
    finally:
        c.close()


def test_the_scenes_do_what_they_are_for(built):
    """behind: nothing is hit; the chains: ray j hits triangle j, every depth in every tile; the soup: hits and misses, and tile pairs of
    48x16 that are split by an octant change (two one-packet walks) beside pairs that are not (the paired walk)"""
    for w, h in [(16, 8)] + FAST_GRIDS + OFF_GRIDS:
        rays, want = scene("behind").rays("mem", w, h)
        assert (want["prim_id"] < 0).all() and (rays["direction"] > 0).all()   # one octant: no generic walk
    for n in (2, 63, 64):
        rays, want = scene(f"chain{n}").rays("mem", 32, 16)
        assert np.array_equal(want["prim_id"], dt.chain_ids(n)[np.arange(512) % n])
        _, want = scene(f"chain{n}").rays("cam", 32, 16)
        assert len(set(want["prim_id"][want["prim_id"] >= 0])) >= 2   # the camera's grid sees more than one depth of the chain
    rays, want = scene("soup").rays("mem", 48, 16)
    hit = want["prim_id"] >= 0
    assert hit.any() and (~hit).any()
    d = rays["direction"].reshape(16, 48, 3)
    kinds = set()
    for ty in range(2):
        for pair in range(3):
            octs = []
            for t in range(2):
                flat = (d[ty * 8:ty * 8 + 8, (2 * pair + t) * 8:(2 * pair + t) * 8 + 8] < 0).reshape(-1, 3)
                octs.append(tuple(flat[0]) if (flat == flat[0]).all() else None)
            assert None not in octs
            kinds.add("paired" if octs[0] == octs[1] else "split")
    assert kinds == {"paired", "split"}


COUNTED = ("rays_cast", "hits", "wave_node_fetches", "wave_tri_fetches", "max_stack_depth", "dead_pops")


def _counted(sc, opts, how, w, h):
    c = capi.Context(0, count_visits=True, **opts)
    try:
        sc.upload(c)
        if how == "tiled":
            rays, want = sc.rays("mem", w, h)
            got, variant = _tiled(c, rays, w, h)
        else:
            rays, want = sc.rays("cam", w, h)
            got = c.cast_grid(capi.camera_look(*sc.camera[:2], w, h, sc.camera[2]), w, h)
            variant = c.last_kernel_variant()
        assert variant.startswith("trace_packet_rows_kernel<false, true, "), variant
        parity.assert_exact(got, want, f"counting {sc.name} {w}x{h} {variant}")
        s = c.stats()
        return {k: s[k] for k in COUNTED}, variant
    finally:
        c.close()


@pytest.mark.parametrize("how,cull", [("tiled", 1), ("grid", 2)], ids=["paired", "culling"])
@pytest.mark.parametrize("name,w,h", [("behind", 16, 8), ("chain2", 32, 16), ("chain63", 32, 16), ("chain64", 32, 16), ("soup", 32, 16), ("soup", 40, 16)])
def test_counting_builds_agree_between_workgroup_sizes_and_with_the_scene(built, name, w, h, how, cull):
    sc = scene(name)
    s64, v64 = _counted(sc, dict(kernel=DUAL, packet_wg=64, packet_cull=cull), how, w, h)
    s256, v256 = _counted(sc, dict(kernel=DUAL, packet_wg=256, packet_cull=cull), how, w, h)
    print(f"COUNTED {name} {w}x{h} {how}: {v64} {s64}")
    assert ", 64, " in v64 and ", 256, " in v256 and s64 == s256, (v64, s64, v256, s256)
    _, want = sc.rays("mem" if how == "tiled" else "cam", w, h)
    assert s64["rays_cast"] == w * h and s64["hits"] == int((want["prim_id"] >= 0).sum())
    assert s64["wave_node_fetches"] >= -(-w // 16) * -(-h // 8)          # every wave fetches the root at least
    if name == "behind":
        assert s64["max_stack_depth"] <= 1 and s64["wave_tri_fetches"] == 0   # nothing pushed: the first pop is the sentinel's
    elif name.startswith("chain"):
        assert s64["max_stack_depth"] == sc.n                            # deep_tree.high_water of a forward ray: n
    else:
        assert s64["max_stack_depth"] >= 3                               # pops in a row happen
        assert s64["max_stack_depth"] <= sc_stack_need(sc)


def sc_stack_need(sc):
    c = capi.Context(0, kernel=DUAL)
    try:
        sc.upload(c)
        return c.scene_info()["stack_need"]
    finally:
        c.close()


def test_the_one_packet_counting_build_matches_the_oracles_counters(built):
    """MRT_KERNEL_PACKET_ROWS, counting (the form whose clock brackets the fetch): the same bounds test_parity_gpu.py holds the row
    kernels to, on the soup at 32x16; the high-water mark of the chains"""
    sc = scene("soup")
    rays, _ = sc.rays("mem", 32, 16)   # (as 8x8 tiles: each of one octant, so each packet takes the one-packet loop)
    want, ctr = sc.osc.trace(rays, counters=True)
    c = capi.Context(0, kernel=ROWS, count_visits=True)
    try:
        sc.upload(c)
        got, variant = _tiled(c, rays, 32, 16)
        parity.assert_exact(got, want, "counting one-packet soup")
        assert variant == "trace_packet_rows_kernel<false, true, 1, 256, false>", variant
        s = c.stats()
        n_packets = rays.shape[0] // 64
        assert s["rays_cast"] == rays.shape[0] and s["hits"] == ctr["hits"]
        assert ctr["node_visits"] / rays.shape[0] <= s["wave_node_fetches"] / n_packets
        assert 0 < s["wave_node_fetches"] <= ctr["node_visits"] and 0 < s["wave_tri_fetches"] <= ctr["tri_tests"] * 64
        assert 3 <= s["max_stack_depth"] <= c.scene_info()["stack_need"]
    finally:
        c.close()
    for n in (2, 63, 64):
        sc = scene(f"chain{n}")
        rays, want = sc.rays("mem", 32, 16)
        c = capi.Context(0, kernel=ROWS, count_visits=True)
        try:
            sc.upload(c)
            parity.assert_exact(c.cast(rays, flags=capi.FLAG_COHERENT), want, f"counting one-packet chain({n})")
            assert c.stats()["max_stack_depth"] == n
        finally:
            c.close()
