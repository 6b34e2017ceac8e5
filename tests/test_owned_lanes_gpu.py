"""The box and triangle tests of the 128-ray walk on owning lanes only (csrc/packet_rows_kernel.h, -DMRT_ROWS_OWNEXEC=1): in such a
build a group's tests run with EXEC narrowed to the lanes that own the row (plus lane 0 at a node), in the default build on all 64
(DESIGN 4.1b round 8 says why).  These tests hold either build (MRT_LIB_PATH names the library): every record bit for bit against
the oracle, outputs poisoned before each cast, on the scenes and forms of test_packed_slab_gpu.py (imported, not copied) and on the
cases this change can break:

  lane0     small triangles only before columns 5..7 of tile A and columns 8..10 of tile B of a 16x8 grid, none on a ray of either
            group's lane 0: both children of the upper rows are hit by lanes other than lane 0, which still has to keep the
            near / far decision's operands current;
  empty_b   small triangles before tile A only: group B hits nothing and owns no row the triangles hang under;
  soup      at 17x9 and at 13x5: clipped grids, group B's tile partly or wholly absent (the general code: the entry EXEC kept in a
            scalar pair);
  single    test_packed_slab_gpu.py's tree of two leaves, with one ray of 128 left of x = 12.2: each leaf is owned by that single
            lane, which replaces its best hit eight times and then takes the exact tie for the lower id.

The walk order must not move: the counting build's figures on every case are held to tests/golden/owned_lanes_counters.json, taken
from the default build, so a switch-on library passes only with the same node fetches, triangle fetches, stack depth, dead pops and
hits (counting builds walk on the general code)."""
import json
import os

import numpy as np
import pytest

import parity
import test_packed_slab_gpu as ps
from messyerraytracer_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "owned_lanes_counters.json")
LANE0_PIXELS = {0: [(5, 1), (6, 2), (7, 5), (5, 6), (6, 3), (7, 4)], 1: [(0, 1), (1, 2), (2, 5), (0, 6), (1, 3), (2, 4)]}
SINGLE_PIXEL = (5, 3)   # tile A, not lane 0


def _pixel_triangles(pixels_by_tile):
    """one small triangle on the ray of each listed pixel of OFF_AXIS's 16x8 grid, at growing distances (as ps._cluster_verts)"""
    rays = po.grid_rays(*ps.OFF_AXIS[:2], 16, 8, ps.OFF_AXIS[2]).reshape(8, 16)
    v = []
    for tile, pixels in pixels_by_tile.items():
        for k, (px, py) in enumerate(pixels):
            r = rays[py, 8 * tile + px]
            c = r["origin"] + np.float32(6.0 + 1.5 * k) * r["direction"]
            s = np.float32(0.02)
            v.append([c + [-s, -s, 0], c + [s, -s, 0], c + [0, s, 0]])
    return np.float32(v)


def _verts_scene(name, v):
    s = ps.Scene.__new__(ps.Scene)
    s.name, s.cache, s.tree = name, {}, None
    n = v.shape[0]
    s.v, s.ids, s.layers = v, (7 * n - 3 * np.arange(n)).astype(np.uint32), (1 << (np.arange(n) % 3)).astype(np.uint32)
    s.osc = po.OracleScene(v, s.ids, s.layers)
    return s


def _single_scene():
    """ps's `replaced` tree under rays of which one alone (SINGLE_PIXEL) starts left of x = 12.2"""
    s = ps.Scene("replaced")
    s.name = "single"
    gx, gy = np.meshgrid(np.arange(16) + 0.5, np.arange(8) + 0.5, indexing="xy")
    x = gx + 13.0
    x[SINGLE_PIXEL[1], SINGLE_PIXEL[0]] = 3.5
    rays = np.ascontiguousarray(ps._rays(np.stack([x.ravel(), gy.ravel(), np.full(128, -3.0)], axis=1), [0.0, 0.0, 1.0]))
    s.cache[(None, 16, 8)] = (rays, s.trace(rays))
    return s


OWN_CASES = {
    "lane0": [(ps.OFF_AXIS, 16, 8)],
    "empty_b": [(ps.OFF_AXIS, 16, 8)],
    "soup": [(ps.OFF_AXIS, 17, 9), (ps.OFF_AXIS, 13, 5)],
    "single": [(None, 16, 8)],
}
_OWN = {}


def own_scene(name):
    if name == "soup":
        return ps.scene("soup")
    if name not in _OWN:
        _OWN[name] = (_single_scene() if name == "single" else
                      _verts_scene(name, _pixel_triangles(LANE0_PIXELS if name == "lane0" else {0: LANE0_PIXELS[0] + [(1, 1), (2, 6)]})))
    return _OWN[name]


# (where the scene comes from, its name, its cases)
ALL = [(ps.scene, n, k) for n, k in ps.CASES.items()] + [(own_scene, n, k) for n, k in OWN_CASES.items()]
IDS = ["packed-" + n for n in ps.CASES] + ["own-" + n for n in OWN_CASES]


@pytest.mark.parametrize("form", list(ps.FORMS))
@pytest.mark.parametrize("which", ALL, ids=IDS)
def test_every_scene_on_every_form(built, which, form):
    get, name, all_cases = which
    opts, how, tail = ps.FORMS[form]
    sc = get(name)
    cases = [k for k in all_cases if how == "tiled" or k[0] is not None]
    if not cases:
        return   # (the culling loop is reached through a camera; this scene's rays are its own)
    c = capi.Context(0, **opts)
    try:
        sc.upload(c)
        for cam, w, h in cases:
            ps._cast_form(c, sc, how, tail, cam, w, h)
    finally:
        c.close()


def test_the_new_scenes_do_what_they_are_for(built):
    rays, want = own_scene("lane0").rays(ps.OFF_AXIS, 16, 8)
    octs = ps._octants(rays, 16, 8)
    assert octs[0] is not None and octs[0] == octs[1]   # one paired walk
    prim = want["prim_id"].reshape(8, 16)
    assert prim[0, 0] == -1 and prim[0, 8] == -1        # the two rays of lane 0
    assert (prim[:, :5] == -1).all() and (prim[:, 11:] == -1).all()
    assert (prim[:, 5:8] >= 0).sum() >= 4 and (prim[:, 8:11] >= 0).sum() >= 4
    _, want = own_scene("empty_b").rays(ps.OFF_AXIS, 16, 8)
    prim = want["prim_id"].reshape(8, 16)
    assert (prim[:, 8:] == -1).all() and (prim[:, :8] >= 0).sum() >= 5
    for w, h in ((17, 9), (13, 5)):
        rays, want = own_scene("soup").rays(ps.OFF_AXIS, w, h)
        d = rays["direction"] < 0
        assert (d == d[0]).all() and (want["prim_id"] >= 0).any() and (want["prim_id"] < 0).any(), (w, h)
    sc = own_scene("single")
    rays, want = sc.rays(None, 16, 8)
    prim = want["prim_id"].reshape(8, 16)
    alone = np.zeros((8, 16), bool)
    alone[SINGLE_PIXEL[1], SINGLE_PIXEL[0]] = True
    assert (prim[alone] == 20).all() and (prim[~alone] == -1).all() and want["t"].reshape(8, 16)[alone][0] == np.float32(3.5)
    assert want.tobytes() == po.trace_brute(sc.tree[0], rays).tobytes()


def counted_figures():
    """case -> the counting build's figures on the paired walk (64-thread workgroups), for every tiled case of every scene"""
    out = {}
    for get, name, all_cases in ALL:
        for i, (cam, w, h) in enumerate(all_cases):
            s, variant, _ = ps._counted(get(name), dict(kernel=ps.DUAL, packet_wg=64, packet_cull=1), cam, w, h)
            out[f"{get.__name__}:{name}:{i}:{w}x{h}"] = {k: int(v) for k, v in s.items()}
    return out


def test_the_walk_order_did_not_move(built):
    got = counted_figures()
    for k in sorted(got):
        print("COUNTED", k, json.dumps(got[k], sort_keys=True))
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong
