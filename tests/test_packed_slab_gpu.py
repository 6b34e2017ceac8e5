"""The node step of the 128-ray walk on rows that both ray groups of a wave own (csrc/packet_rows_kernel.h).  In builds with
-DMRT_ROWS_PKSLAB=1 the child boxes of such a row are tested with v_pk_fma_f32 on {group A, group B} register pairs
(MRT_ROWSW_PKSLAB) and a row only one group owns takes the single-group test out of line; the default build tests the groups one
after the other (DESIGN 4.1b round 7 says why).  These tests hold either build (MRT_LIB_PATH names the library).  Every record bit
for bit against the oracle, outputs poisoned before each cast.

  soup      300 triangles across both tiles of a wave: rows both groups own at every depth (16x8: one wave pair; 32x16: four
            waves of four octants, from the front and from the back: all eight; 48x8: the middle pair is split by the sign
            change of dx and takes the one-packet loop; 20x12: clipped tiles on the general code);
  clusters  a few small triangles in front of each tile of a 16x8 grid: every row below the root is owned by one group, the
            single-group test runs beside the paired one in the same walk;
  replaced  a caller's tree of two leaves under loose boxes, eight parallel triangles listed far to near and a coplanar pair
            listed higher id first: every hitting lane replaces its best hit eight times and then takes the exact tie for the
            lower id; the lanes right of x = 12.2 never hit and must hold the miss record;
  one       a one-triangle scene: a wrapped root leaf, its padding box with non-finite planes goes through the node step;
  graze     axis-parallel rays in the face planes of leaf and inner boxes of a tiled wall (test_parity_gpu.py's graze test,
            arranged as a 32x16 grid of one octant);
  chain16, chain64   deep_tree's chain: the stack at its bound (64) and well below it.

Forms: the paired walk on the whole-tile fast path and on the general code, 64- and 256-thread workgroups; the culling loop
(camera scenes, through mrt_cast_grid); closest hit, any hit and tokens on each; the counting build."""
import numpy as np
import pytest

import deep_tree as dt
from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
import parity

pytestmark = pytest.mark.gpu
DUAL = capi.KERNEL_PACKET_DUAL
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
ORIGIN = (0.0, 0.0, -12.0)
OFF_AXIS = ((-7.0, -7.0, -7.0), (3.0 ** -0.5,) * 3, 30.0)   # through the soup's middle, so narrow that every ray shares one octant
ALONG_Z = (ORIGIN, (0.0, 0.0, 1.0), 50.0)         # dx and dy change sign at the image centre
BACK = ((0.0, 0.0, 12.0), (0.0, 0.0, -1.0), 50.0)  # the other four octants
TILTED = (ORIGIN, (0.0, 0.6, 1.0), 30.0)          # dy keeps its sign over eight rows, dx changes at the centre
N_SOUP = 300

# form -> (context options, how the rays get there, the instantiation's template arguments after <any hit, counting,)
FORMS = {
    "pair_fast_wg64": (dict(kernel=DUAL, packet_wg=64, packet_cull=1), "tiled", "2, 64, false>"),
    "pair_fast_wg256": (dict(kernel=DUAL, packet_wg=256, packet_cull=1), "tiled", "2, 256, false>"),
    "pair_general_wg64": (dict(kernel=DUAL, packet_wg=64, packet_cull=1, tile_order=3), "tiled", "2, 64, false>"),
    "pair_general_wg256": (dict(kernel=DUAL, packet_wg=256, packet_cull=1, tile_order=3), "tiled", "2, 256, false>"),
    "cull_wg64": (dict(kernel=DUAL, packet_wg=64, packet_cull=2), "grid", "2, 64, true>"),
    "cull_wg256": (dict(kernel=DUAL, packet_wg=256, packet_cull=2), "grid", "2, 256, true>"),
}
# scene -> [(camera or None = the scene's own rays, width, rows)]
CASES = {
    "soup": [(OFF_AXIS, 16, 8), (ALONG_Z, 32, 16), (BACK, 32, 16), (TILTED, 48, 8), (ALONG_Z, 20, 12)],
    "clusters": [(OFF_AXIS, 16, 8)],
    "replaced": [(None, 16, 8)],
    "one": [(OFF_AXIS, 16, 8), (ALONG_Z, 32, 16)],
    "graze": [(None, 32, 16)],
    "chain16": [(None, 32, 16), ("chain", 32, 16)],
    "chain64": [(None, 32, 16), ("chain", 32, 16)],
}


def _rays(origins, direction):
    r = np.zeros(len(origins), dtype=T.RAY32)
    r["origin"] = np.asarray(origins, dtype=np.float32)
    r["direction"] = np.asarray(direction, dtype=np.float32)
    r["t_min"], r["t_max"] = 0.001, T.FLT_MAX
    return r


def _cluster_verts():
    """six small triangles on rays of tile A (columns 0..7) and six on rays of tile B of OFF_AXIS's 16x8 grid"""
    rays = po.grid_rays(*OFF_AXIS[:2], 16, 8, OFF_AXIS[2]).reshape(8, 16)
    v = []
    for tile in range(2):
        for k, (px, py) in enumerate([(1, 1), (5, 2), (2, 5), (6, 6), (3, 3), (4, 6)]):
            r = rays[py, 8 * tile + px]
            c = r["origin"] + np.float32(6.0 + 1.5 * k) * r["direction"]
            s = np.float32(0.02)
            v.append([c + [-s, -s, 0], c + [s, -s, 0], c + [0, s, 0]])
    return np.float32(v)


def _replaced_scene():
    """(tris, nodes, prim_idx): the root over two leaves that both carry the box of everything (so the walk cannot cull by them, and
    with equal entry distances it takes the right leaf first): right = the planes z = 8, 7, 6, 5 in that order, left = z = 4, 3, 2, 1
    and the coplanar pair at z = 0.5, the higher id first"""
    zs = [4.0, 3.0, 2.0, 1.0, 0.5, 0.5, 8.0, 7.0, 6.0, 5.0]
    verts = np.float32([[[12.2, -100.0, z], [12.2, 100.0, z], [-100.0, 0.0, z]] for z in zs])
    ids = np.uint32([140, 130, 120, 110, 50, 20, 180, 170, 160, 150])
    tris = capi.make_triangles(verts, ids, np.full(10, 1, np.uint32))
    nodes = np.zeros(4, dtype=T.NODE32)
    nodes["aabb_min"][[0, 2, 3]], nodes["aabb_max"][[0, 2, 3]] = [-100.0, -100.0, 0.5], [12.2, 100.0, 8.0]
    nodes["left_first"][0], nodes["tri_count"][0] = 2, 0
    nodes["left_first"][2], nodes["tri_count"][2] = 0, 6
    nodes["left_first"][3], nodes["tri_count"][3] = 6, 4
    return tris, nodes, np.arange(10, dtype=np.uint32)


def _wall(n=8, pitch=1.0):
    """test_parity_gpu.py's tiled wall: every triangle edge on a multiple of the pitch, i.e. on faces of leaf and inner boxes"""
    tris = []
    for z, off in ((0.0, 0.0), (1.5 * pitch, 0.5)):
        for i in range(n):
            for j in range(n):
                x0, y0, x1, y1 = (i + off) * pitch, (j + off) * pitch, (i + off + 1) * pitch, (j + off + 1) * pitch
                a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
                tris += [(a, b, c), (a, c, d)]
    return np.array(tris, dtype=np.float32)


class Scene:
    """a scene, its rays per case and the expected records, made once and never changed"""

    def __init__(self, name):
        self.name, self.cache, self.tree = name, {}, None
        if name.startswith("chain"):
            self.n = int(name[5:])
            s = dt.prepared(self.n)
            self.tree = (s["tris"], s["nodes"], s["prim_idx"])
        elif name == "replaced":
            self.tree = _replaced_scene()
        else:
            if name == "soup":
                v = synth.soup(N_SOUP, 1.2, 5)
            elif name == "clusters":
                v = _cluster_verts()
            elif name == "one":
                v = np.float32([[[-6, -6, 2], [9, -5, 3], [0, 8, 1]]])
            else:
                v = _wall()
            n = v.shape[0]
            self.v, self.ids, self.layers = v, (7 * n - 3 * np.arange(n)).astype(np.uint32), (1 << (np.arange(n) % 3)).astype(np.uint32)
            self.osc = po.OracleScene(v, self.ids, self.layers)
        if self.tree is not None:
            self.wide, self.leaf_tris = po.to_wide(*self.tree)

    def upload(self, c):
        if self.tree is not None:
            c.upload_scene(*self.tree)
        else:
            capi.Scene(self.v, self.ids, self.layers).upload(c)

    def trace(self, rays, **kw):
        return po.trace(self.wide, self.leaf_tris, rays, **kw) if self.tree is not None else self.osc.trace(rays, **kw)

    def camera(self, cam):
        return dt.grid_camera(self.n) if cam == "chain" else cam

    def rays(self, cam, w, h):
        key = (cam, w, h)
        if key not in self.cache:
            if cam is not None:
                cm = self.camera(cam)
                rays = po.grid_rays(*cm[:2], w, h, cm[2])
            elif self.name.startswith("chain"):
                rays = np.ascontiguousarray(dt.forward_rays(self.n, w * h))
            elif self.name == "replaced":   # along +z from pixel centres of [0, 16) x [0, 8)
                gx, gy = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5, indexing="xy")
                rays = _rays(np.stack([gx.ravel(), gy.ravel(), np.full(w * h, -3.0)], axis=1), [0.0, 0.0, 1.0])
            else:                           # graze: the upper half along +z from points on tile edges, the lower half along +x inside the walls' planes
                xs = (np.arange(w) * 0.25).astype(np.float32)
                gx, gy = np.meshgrid(xs, xs[:h // 2], indexing="xy")
                rays = np.concatenate([_rays(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -3.0)], axis=1), [0.0, 0.0, 1.0]),
                                       _rays(np.stack([np.full(gx.size, -2.0), gx.ravel(), np.where(gy.ravel() % 0.5 == 0, 0.0, 1.5)], axis=1), [1.0, 0.0, 0.0])])
            self.cache[key] = (np.ascontiguousarray(rays), self.trace(rays))
        return self.cache[key]


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = Scene(name)
    return _SCENES[name]


def _octants(rays, w, h):
    """per 8x8 tile (row-major over whole tiles): the tile's octant as a tuple, or None if its rays do not share one"""
    d = rays["direction"].reshape(h, w, 3)
    out = []
    for ty in range(h // 8):
        for tx in range(w // 8):
            flat = (d[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] < 0).reshape(-1, 3)
            out.append(tuple(flat[0]) if (flat == flat[0]).all() else None)
    return out


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


def _tokens(c, rays, n, what, want):
    """mrt_cast(COHERENT) of device rays to tokens, then the records rebuilt from them"""
    d_rays, d_tok, d_hits = c.device_alloc(n * 32), c.device_alloc(n * 4), c.device_alloc(n * 32)
    try:
        c.h2d(d_rays, rays)
        c.h2d(d_tok, np.full(n * 4, 0xA5, np.uint8))
        c.h2d(d_hits, np.full(n * 32, 0xA5, np.uint8))
        c.cast(d_rays, d_tok, count=n, flags=capi.FLAG_COHERENT | DEV | capi.FLAG_TOKEN_OUT)
        variant = c.last_kernel_variant()
        tok = np.zeros(n, np.uint32)
        c.d2h(tok, d_tok)
        assert np.array_equal(tok != capi.TOKEN_MISS, want["prim_id"] >= 0), f"{what}: tokens"
        c.expand_tokens(d_rays, d_tok, d_hits, n)
        c.synchronize()
        rec = np.zeros(n, dtype=T.HIT32)
        c.d2h(rec, d_hits)
    finally:
        c.device_free(d_rays); c.device_free(d_tok); c.device_free(d_hits)
    parity.assert_exact(rec, want, what + ": records rebuilt from the tokens")
    return variant


def _check_any(a, want, what):
    """any-hit records: SOME hit of every ray that has one; the closest triangle's record where that is the one found"""
    hit = want["prim_id"] >= 0
    assert np.array_equal(a["prim_id"] >= 0, hit) and (a["t"][hit] >= want["t"][hit]).all(), f"{what}: any-hit records"
    same = hit & (a["prim_id"] == want["prim_id"])
    assert a[same].tobytes() == want[same].tobytes(), f"{what}: any-hit records of the closest triangle"


def _cast_form(c, sc, how, tail, cam, w, h):
    what = f"{sc.name} {w}x{h} {tail}"
    rays, want = sc.rays(cam, w, h)
    if how == "tiled":
        got, variant = _tiled(c, rays, w, h)
        assert variant == "trace_packet_rows_kernel<false, false, " + tail, (what, variant)
        parity.assert_exact(got, want, what)
        a, variant = _tiled(c, rays, w, h, mode=capi.MODE_ANY_HIT)
        assert variant == "trace_packet_rows_kernel<true, false, " + tail, (what, variant)
        _check_any(a, want, what)
        if w * h >= 256:   # (a smaller cast is not the packet walks')
            variant = _tokens(c, rays, w * h, what, want)
            assert variant.startswith("trace_packet_rows_kernel<false, false, 2, "), (what, variant)
    else:
        cm = sc.camera(cam)
        look = capi.camera_look(*cm[:2], w, h, cm[2])
        got = c.cast_grid(look, w, h)
        assert c.last_kernel_variant() == "trace_packet_rows_kernel<false, false, " + tail, (what, c.last_kernel_variant())
        parity.assert_exact(got, want, what)
        lit = c.cast_grid(look, w, h, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        assert c.last_kernel_variant() == "trace_packet_rows_kernel<true, false, " + tail, (what, c.last_kernel_variant())
        assert np.array_equal(lit.astype(bool), want["prim_id"] >= 0), f"{what}: any-hit bools"
        tok = c.cast_grid(look, w, h, flags=capi.FLAG_TOKEN_OUT)
        assert c.last_kernel_variant() == "trace_packet_rows_kernel<false, false, " + tail, (what, c.last_kernel_variant())
        assert np.array_equal(tok != capi.TOKEN_MISS, want["prim_id"] >= 0), f"{what}: tokens"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_every_scene_on_every_form(built, name, form):
    opts, how, tail = FORMS[form]
    sc = scene(name)
    cases = [k for k in CASES[name] if how == "tiled" or k[0] is not None]
    if not cases:
        return   # (the culling loop is reached through a camera; this scene's rays are its own)
    c = capi.Context(0, **opts)
    try:
        sc.upload(c)
        for cam, w, h in cases:
            _cast_form(c, sc, how, tail, cam, w, h)
    finally:
        c.close()


def test_the_scenes_do_what_they_are_for(built):
    soup = scene("soup")
    for cam, w, h in CASES["soup"]:
        rays, want = soup.rays(cam, w, h)
        hit = want["prim_id"] >= 0
        assert hit.any() and (~hit).any(), (w, h)
    # one wave pair of one octant with hits in both tiles; four waves of four octants; 48x8: a split pair between two paired ones
    rays, want = soup.rays(OFF_AXIS, 16, 8)
    octs = _octants(rays, 16, 8)
    assert octs[0] is not None and octs[0] == octs[1]
    hit = (want["prim_id"] >= 0).reshape(8, 16)
    assert hit[:, :8].any() and hit[:, 8:].any()
    octs = _octants(soup.rays(ALONG_Z, 32, 16)[0], 32, 16)
    back = _octants(soup.rays(BACK, 32, 16)[0], 32, 16)
    for o in (octs, back):
        assert None not in o and all(o[i] == o[i + 1] for i in (0, 2, 4, 6))
    assert len(set(octs) | set(back)) == 8
    octs = _octants(soup.rays(TILTED, 48, 8)[0], 48, 8)
    assert None not in octs and octs[0] == octs[1] and octs[2] != octs[3] and octs[4] == octs[5]
    # clusters: each tile hits its own triangles only, and some lanes of each hit nothing
    rays, want = scene("clusters").rays(OFF_AXIS, 16, 8)
    ids = scene("clusters").ids
    prim = want["prim_id"].reshape(8, 16)
    for tile in range(2):
        seen = set(int(i) for i in prim[:, 8 * tile:8 * tile + 8].ravel())
        assert -1 in seen and seen <= {-1} | set(int(i) for i in ids[6 * tile:6 * tile + 6]) and len(seen) >= 4, (tile, seen)
    # replaced: the lower id of the coplanar pair where a ray hits, the miss record right of x = 12.2
    rays, want = scene("replaced").rays(None, 16, 8)
    prim = want["prim_id"].reshape(8, 16)
    assert (prim[:, :12] == 20).all() and (prim[:, 13:] == -1).all() and (want["t"][want["prim_id"] == 20] == np.float32(3.5)).all()
    assert want.tobytes() == po.trace_brute(scene("replaced").tree[0], rays).tobytes()
    # one: hits and misses; graze: both; the chains: ray j hits triangle j
    for name, cam, w, h in (("one", OFF_AXIS, 16, 8), ("one", ALONG_Z, 32, 16), ("graze", None, 32, 16)):
        _, want = scene(name).rays(cam, w, h)
        assert (want["prim_id"] >= 0).any() and (want["prim_id"] < 0).any(), name
    for n in (16, 64):
        rays, want = scene(f"chain{n}").rays(None, 32, 16)
        assert np.array_equal(want["prim_id"], dt.chain_ids(n)[np.arange(512) % n])
        assert want.tobytes() == po.trace_brute(scene(f"chain{n}").tree[0], rays).tobytes()


COUNTED = ("rays_cast", "hits", "wave_node_fetches", "wave_tri_fetches", "max_stack_depth", "dead_pops")


def _counted(sc, opts, cam, w, h):
    c = capi.Context(0, count_visits=True, **opts)
    try:
        sc.upload(c)
        rays, want = sc.rays(cam, w, h)
        got, variant = _tiled(c, rays, w, h)
        assert variant.startswith("trace_packet_rows_kernel<false, true, 2, "), variant
        parity.assert_exact(got, want, f"counting {sc.name} {w}x{h} {variant}")
        s = c.stats()
        return {k: s[k] for k in COUNTED}, variant, c.scene_info()["stack_need"]
    finally:
        c.close()


def test_the_counting_build_matches_the_oracles_counters(built):
    """the soup at 32x16 on the counting build of the paired walk: the bounds test_parity_gpu.py holds the packet walks' counters to
    against the oracle's own (a packet fetches at least what its hungriest ray needs and at most what its 128 rays need together), the
    same figures from both workgroup sizes; printed, so that two builds of the library can be compared figure for figure"""
    sc = scene("soup")
    rays, _ = sc.rays(ALONG_Z, 32, 16)
    want, ctr = sc.trace(rays, counters=True)
    s64, v64, need = _counted(sc, dict(kernel=DUAL, packet_wg=64, packet_cull=1), ALONG_Z, 32, 16)
    s256, v256, _ = _counted(sc, dict(kernel=DUAL, packet_wg=256, packet_cull=1), ALONG_Z, 32, 16)
    print(f"COUNTED soup 32x16: {v64} {s64}")
    assert ", 64, " in v64 and ", 256, " in v256 and s64 == s256, (v64, s64, v256, s256)
    n_packets = rays.shape[0] // 64
    assert s64["rays_cast"] == rays.shape[0] and s64["hits"] == ctr["hits"] == int((want["prim_id"] >= 0).sum())
    assert ctr["node_visits"] / rays.shape[0] <= s64["wave_node_fetches"] / n_packets * 2
    assert 0 < s64["wave_node_fetches"] <= ctr["node_visits"] and 0 < s64["wave_tri_fetches"] <= ctr["tri_tests"] * 64
    assert 3 <= s64["max_stack_depth"] <= need
    for n in (16, 64):   # the chains: the stack's high-water mark is the tree's depth
        s, _, need = _counted(scene(f"chain{n}"), dict(kernel=DUAL, packet_wg=64, packet_cull=1), None, 32, 16)
        assert s["max_stack_depth"] == n == need
