"""The chain scene (tests/deep_tree.py) without a device: the library's host preparation of a caller's tree as deep as it has
triangles is a clean layout with depth == n; the oracle's walk over those very nodes equals the brute-force test of every triangle on
every ray of every set (no ray left out), so the scene is a fair input for the GPU tier; and the push rules of the walks, restated in
Python over the prepared nodes, reach exactly n entries on the 2-wide tree -- the expected max_stack_depth of test_deep_trees_gpu.py,
from something other than a kernel."""
import numpy as np
import pytest

import deep_tree as dt
import layout_check as lc
from oracle import pyoracle as po

DEPTHS = [2, 8, 9, 16, 17, 63, 64]
# the most entries a 4- / 8-wide walk holds on chain(n) (no sentinel: the persistent kernels keep none), by the restatement below:
# every node but the last has one inner child and 3 (7) leaves, and a forward ray from x = 0 pushes all the leaves
WIDE_HIGH_WATER = {2: (1, 1), 8: (7, 7), 9: (8, 8), 16: (15, 15), 17: (16, 16), 63: (62, 62), 64: (63, 63)}


def ray_sets(n):
    o, f, fov = dt.grid_camera(n)
    return {"axis": dt.axis_rays(n), "interleaved": dt.interleaved_rays(n), "bounded": dt.bounded_rays(n),
            "grid": po.grid_rays(o, f, dt.GRID_W, dt.GRID_H, fov)}


@pytest.mark.parametrize("n", DEPTHS)
def test_chain_is_a_clean_layout_of_depth_n(built, n):
    s = dt.prepared(n)
    snap = s["snap"]
    findings = lc.check_flat(snap, s["tris"], leaf_boxes="host", nodes32=s["nodes"])
    assert not findings, lc.summary(findings)
    assert snap["depth"] == n and snap["n_nodes"] == n - 1
    assert snap["nodes4"] is not None and snap["nodes8"] is not None
    assert (snap["tri_hot"]["id"] != np.arange(n)).all() and set(snap["tri_hot"]["layers"]) == {1, 2}
    if n == 64:
        assert (snap["n_nodes"], snap["n_nodes4"], snap["n_nodes8"]) == (63, 21, 9)


@pytest.mark.parametrize("n", DEPTHS)
def test_walk_over_the_chain_equals_brute_force_on_every_ray(built, n):
    s = dt.prepared(n)
    for name, rays in ray_sets(n).items():
        for mask in (0xFFFFFFFF, dt.LAYERS[1]):   # all triangles; the odd ones only
            want = po.trace_brute(s["tris"], rays, query_mask=mask)
            got = po.trace(s["wide"], s["leaf_tris"], rays, query_mask=mask)
            assert got.tobytes() == want.tobytes(), (n, name, hex(mask))
            lit = po.trace(s["wide"], s["leaf_tris"], rays, query_mask=mask, any_hit=True)
            assert np.array_equal(lit["prim_id"] >= 0, want["prim_id"] >= 0), (n, name, hex(mask))
    want = po.trace_brute(s["tris"], dt.axis_rays(n))
    ids = dt.chain_ids(n)
    assert np.array_equal(want["prim_id"][:n], ids), "forward ray j hits triangle j"
    assert (want["prim_id"][n:] == ids[n - 1]).all(), "every backward ray hits the last triangle"
    assert np.allclose(want["t"][:n], np.arange(1, n + 1), rtol=1e-6, atol=0), "... in its plane x = j + 1"
    masked = po.trace_brute(s["tris"], dt.forward_rays(n), query_mask=dt.LAYERS[1])["prim_id"]
    k = np.arange(n) | 1
    assert np.array_equal(masked, np.where(k < n, ids[np.minimum(k, n - 1)].astype(np.int64), -1)), \
        "with the even triangles masked out ray j hits the next odd triangle: one entry further down"
    bounded = po.trace_brute(s["tris"], dt.bounded_rays(n))
    assert (bounded["prim_id"][:n][1::2] == -1).all(), "t_max ends before the plane"
    assert np.array_equal(bounded["prim_id"][:n - 1][0::4], ids[1:][0::4]), "t_min starts behind the plane: the next triangle"
    assert (bounded["prim_id"][n:][0::4] == -1).all(), "t_max ends before the first plane met"
    odd = np.arange(n)[1::2]   # t_min behind the last plane: triangle n - 2, which holds the points of the rays j <= n - 2
    assert np.array_equal(bounded["prim_id"][n:][1::2], np.where(odd <= n - 2, int(ids[n - 2]), -1))
    grid = po.trace_brute(s["tris"], ray_sets(n)["grid"])
    # (the grid opens from its apex: it reaches y + z <= s_k only for the triangles of the far half and a few before them)
    assert len(set(grid["prim_id"])) >= n // 2, "the grid's answers come from many stack entries"


@pytest.mark.parametrize("n", DEPTHS)
def test_push_rules_restated_reach_the_bound(built, n):
    s = dt.prepared(n)
    snap = s["snap"]
    fwd, back = dt.forward_rays(n), dt.backward_rays(n)
    assert dt.high_water(s["children"][2], fwd[0], s["slot_t"]) == n == snap["depth"]
    assert all(dt.high_water(s["children"][2], r, s["slot_t"]) == min(2, n) for r in back)
    sets = ray_sets(n)
    assert dt.batch_high_water(s, 2, sets["axis"]) == n and dt.batch_high_water(s, 2, sets["interleaved"]) == n
    assert dt.batch_high_water(s, 2, sets["grid"][::97]) == n, "a grid ray crosses every box"
    # bounded rays: forward ray 2 is the deepest unbounded one left (ray 0 starts behind triangle 0's plane and skips its leaf)
    assert dt.batch_high_water(s, 2, sets["bounded"]) == (n if n > 2 else 1)
    h4 = dt.batch_high_water(s, 4, sets["axis"], sentinel=0)
    h8 = dt.batch_high_water(s, 8, sets["axis"], sentinel=0)
    print(f"chain({n}): depth {snap['depth']} stack4 {snap['stack4']} stack8 {snap['stack8']}; restated high water 2-wide {n}, "
          f"4-wide {h4}, 8-wide {h8} (entries above an empty bottom)")
    assert h4 < snap["stack4"] and h8 < snap["stack8"], "stack4 / stack8 count one entry more than a walk can hold"
    assert (h4, h8) == WIDE_HIGH_WATER[n]
    assert snap["stack4"] <= 128 and snap["stack8"] <= 128


def test_chain_65_is_one_deeper_than_the_stacks(built):
    assert dt.prepared(65)["snap"]["depth"] == 65
