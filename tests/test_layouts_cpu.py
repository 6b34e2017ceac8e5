"""The structural validator (tests/layout_check.py) on the CPU: clean layouts pass, and every corruption of a clean layout is
reported under the rule it breaks.  No device: the layouts are the library's own host preparations -- mrt_scene_prepare_host (the
arrays mrt_upload_scene uploads: 2-wide nodes, the 4-wide and the 8-wide collapse with leaf_box, triangles) and
mrt_two_level_prepare_host -- so the 4- and 8-wide mutations start from what the library really builds, not from a numpy
re-derivation.  The row arrays and the parent table exist only on the device; here they are built by the validator's own
restatement (layout_check.expected_rows / expected_parents), which the GPU tier holds to the device's arrays."""
import numpy as np
import pytest

import layout_check as lc
from messyerraytracer_amd import capi, synth, types as T


def tiled_wall(n=12, pitch=1.0):
    """test_parity_gpu._tiled_wall: axis-aligned tiles, every box of zero thickness"""
    tris = []
    for z, off in ((0.0, 0.0), (1.5 * pitch, 0.5)):
        for i in range(n):
            for j in range(n):
                x0, y0, x1, y1 = (i + off) * pitch, (j + off) * pitch, (i + off + 1) * pitch, (j + off + 1) * pitch
                a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
                tris += [(a, b, c), (a, c, d)]
    return np.array(tris, dtype=np.float32)


def mixed_magnitudes(n=2000, seed=7):
    """Triangles whose vertices differ in magnitude by up to 10^6 per coordinate: the edges v1 - v0 are ROUNDED differences (in
    synth.soup they are exact, neighbouring floats subtract exactly), so the float64 vertex v0 + e1 is not the input vertex and
    can lie a fraction of an ulp outside the host builder's exact vertex box: the case rule 4 exists for."""
    rng = np.random.default_rng(seed)
    return ((rng.random((n, 3, 3)) - 0.5) * 10.0 ** rng.integers(-3, 4, size=(n, 3, 3))).astype(np.float32)


def host_snapshot(verts9):
    """what Context.debug_snapshot returns after Scene(verts9).upload(ctx), made without a device"""
    scene = capi.Scene(verts9, n_threads=1)
    snap = capi.prepare_scene_host(scene.tris, scene.nodes, scene.prim_idx)
    snap["rows"] = lc.expected_rows(snap["nodes"], snap["tri_hot"], snap["tri_cold"])
    snap["rows4"] = lc.expected_rows4(snap["nodes4"], snap["tri_hot"], snap["tri_cold"])  # from the library's own 4-wide nodes
    out = lc._Out()
    tree = lc.walk2(snap["nodes"], [0], 0, snap["n_nodes"], snap["n_tris"], out)
    snap["parent"] = lc.expected_parents(tree, 0, snap["n_nodes"])
    snap["scene_abs_max"] = np.float32(max(np.abs(snap["bounds_lo"]).max(), np.abs(snap["bounds_hi"]).max()))
    return snap, scene


FLAT_SCENES = {
    "soup1": lambda: synth.soup(1, 0.5, 1), "soup2": lambda: synth.soup(2, 0.5, 2), "soup3": lambda: synth.soup(3, 0.5, 3),
    "soup17": lambda: synth.soup(17, 0.5, 4), "soup1000": lambda: synth.soup(1000, 0.5, 1), "wall": tiled_wall,
    "coincident300": lambda: np.repeat(synth.soup(1, 0.5, 3), 300, axis=0), "mixed": lambda: mixed_magnitudes(),
}


@pytest.mark.parametrize("name", sorted(FLAT_SCENES))
def test_clean_flat_layouts_pass(built, name):
    snap, scene = host_snapshot(FLAT_SCENES[name]())
    findings = lc.check_flat(snap, scene.tris, leaf_boxes="host", nodes32=scene.nodes)
    assert not findings, lc.summary(findings)
    assert snap["nodes4"] is not None and snap["nodes8"] is not None and snap["leaf_box"] is not None
    # rule 4 on the host tree: the baseline the device trees are held to (GPU tier).  0 where the edges are exact differences
    # (the soups, the wall); where they are rounded ("mixed") a float64 vertex v0 + e lies up to half an ulp of the edge outside the
    # exact vertex box, which in ulps of a small box coordinate is a large number
    slack = lc.containment_slack(snap)
    print(f"{name}: containment slack {slack:.6g} ulp")
    assert (slack > 0.0) == (name == "mixed")


def two_level_inputs(name):
    if name == "room":
        return synth.room()
    if name == "multi4":
        return synth.multi_mesh_instances(4, 600, 0.05, 11)
    local, inst = synth.multi_mesh_instances(1, 200, 0.05, 5)
    return local, inst


@pytest.mark.parametrize("name", ["room", "multi4", "one"])
def test_clean_two_level_layouts_pass(built, name):
    local, inst = two_level_inputs(name)
    snap = capi.two_level_prepare_host(local, inst)
    findings = lc.check_two_level(snap, local, inst, leaf_boxes="host")
    assert not findings, lc.summary(findings)


# ---- mutations: one corruption at a time, each reported under its rule -----------------------------------------------------------

def _next(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


def _inner_edge(snap):
    """(node, side) of a node whose child on that side is an inner node"""
    nodes = snap["nodes"]
    for b in range(nodes.shape[0]):
        if nodes["left_idx"][b] < lc.SENT:
            return b, "left"
    raise AssertionError("no inner child")


def _multi_leaf(snap):
    """first slot and length of a leaf of at least two triangles"""
    nodes = snap["nodes"]
    for side in ("left", "right"):
        sel = np.flatnonzero((nodes[f"{side}_idx"] >= lc.LEAF) & (nodes[f"{side}_count"] >= 2))
        if sel.size:
            return int(nodes[f"{side}_idx"][sel[0]] & lc.SENT), int(nodes[f"{side}_count"][sel[0]]), int(sel[0]), side
    raise AssertionError("no leaf of two triangles")


def m_box_in(s):
    b, side = _inner_edge(s)
    s["nodes"][f"{side}_max"][b, 0] = _next(s["nodes"][f"{side}_max"][b, 0], False)


def m_box_out(s):
    b, side = _inner_edge(s)
    s["nodes"][f"{side}_max"][b, 1] = _next(s["nodes"][f"{side}_max"][b, 1], True)


def m_leaf_box_in(s):
    _, _, b, side = _multi_leaf(s)
    s["nodes"][f"{side}_min"][b, 2] = _next(s["nodes"][f"{side}_min"][b, 2], True)


def m_swap_slots(s):
    f, c, _, _ = _multi_leaf(s)
    s["tri_hot"][[f, f + 1]] = s["tri_hot"][[f + 1, f]]
    s["tri_hot"]["flags"][[f, f + 1]] = s["tri_hot"]["flags"][[f + 1, f]]  # the flags stay where the tree wants them


def m_flag_cleared(s):
    f, c, _, _ = _multi_leaf(s)
    s["tri_hot"]["flags"][f + c - 1] = 0


def m_flag_mid_leaf(s):
    f, c, _, _ = _multi_leaf(s)
    s["tri_hot"]["flags"][f] = 1


def m_count_off(s):
    _, _, b, side = _multi_leaf(s)
    s["nodes"][f"{side}_count"][b] -= 1


def m_ref_to_sibling(s):
    nodes = s["nodes"]
    b = int(np.flatnonzero((nodes["left_idx"] < lc.SENT) & (nodes["right_idx"] < lc.SENT))[0])
    nodes["left_idx"][b] = nodes["right_idx"][b]


def m_parent_side(s):
    s["parent"][int(np.flatnonzero(s["parent"] != lc.ROOT_PARENT)[0])] ^= np.uint32(0x80000000)


def m_parent_wrong(s):
    k = np.flatnonzero(s["parent"] != lc.ROOT_PARENT)
    s["parent"][k[0]] = s["parent"][k[-1]]


def m_slot_src_dup(s):
    s["slot_src"][5] = s["slot_src"][6]


def _leaf_child8(s):
    n8 = s["nodes8"]
    w, c = np.nonzero((n8["ref"] >= lc.LEAF) & (np.arange(8)[None, :] < n8["n_children"][:, None]))
    return int(w[0]), int(c[0])


def m_qhi_dec(s):
    w, c = _leaf_child8(s)
    s["nodes8"]["qhi"][w, 0, c] -= 1


def m_qlo_inc(s):
    w, c = _leaf_child8(s)
    s["nodes8"]["qlo"][w, 1, c] += 1


def m_q_loose(s):
    """two grid steps out: still contains, but looser than the collapse can make it"""
    n8 = s["nodes8"]
    w, c = np.nonzero((np.arange(8)[None, :] < n8["n_children"][:, None]) & (n8["qhi"][:, 2, :] < 250))
    n8["qhi"][w[0], 2, c[0]] += 2


def m_leaf_box_shift(s):
    s["leaf_box"][:] = np.roll(s["leaf_box"], 1, axis=0)


def m_box4_parent(s):
    """a 4-wide child's box replaced by the box of the node above it (contains it, but is not the subtree's own)"""
    n4 = s["nodes4"]
    w = int(np.flatnonzero(n4["n_children"] >= 2)[0])
    n4["box"][w, 0, 0:3] = n4["box"][w, :n4["n_children"][w], 0:3].min(axis=0)
    n4["box"][w, 0, 3:6] = n4["box"][w, :n4["n_children"][w], 3:6].max(axis=0)


def m_ref4_wrong_leaf(s):
    n4 = s["nodes4"]
    w, c = np.nonzero((n4["ref"] >= lc.LEAF) & (np.arange(4)[None, :] < n4["n_children"][:, None]))
    n4["ref"][w[0], c[0]] = n4["ref"][w[1], c[1]]


def m_nchildren4(s):
    n4 = s["nodes4"]
    w = int(np.flatnonzero(n4["n_children"] == 4)[0])
    n4["n_children"][w] = 3


def m_stack4_short(s):
    s["stack4"] -= 1


def m_stack8_short(s):
    s["stack8"] -= 1


def m_row_stale_node(s):
    s["rows"][3, 0] ^= np.uint32(1)


def m_row4_stale(s):
    s["rows4"][2 * 5 + 1, 9] ^= np.uint32(1)  # a ref word of 4-wide node 5


def m_row4_stale_box(s):
    s["rows4"][2 * 7, 3] ^= np.uint32(1)


def m_row_stale_tri(s):
    s["rows"][s["n_nodes"] + 7, 4] ^= np.uint32(1)


def m_depth_short(s):
    s["depth"] -= 1


def m_bounds(s):
    s["bounds_hi"][0] = _next(s["bounds_hi"][0], True)


def m_vertex(s):
    s["tri_hot"]["e1"][11, 0] = _next(s["tri_hot"]["e1"][11, 0], True)


def m_normal(s):
    s["tri_cold"]["normal"][11, 1] = _next(s["tri_cold"]["normal"][11, 1], False)


FLAT_MUTATIONS = [  # (name, corruption, the rule that must report it)
    ("box face inwards by one ulp", m_box_in, 2), ("box face outwards by one ulp", m_box_out, 2),
    ("leaf box face inwards by one ulp", m_leaf_box_in, 3),
    ("two slots swapped in tri_hot only", m_swap_slots, 5), ("kLastInLeaf cleared", m_flag_cleared, 1), ("flag set mid-leaf", m_flag_mid_leaf, 1),
    ("count off by one", m_count_off, 1), ("child ref to the sibling's subtree", m_ref_to_sibling, 1),
    ("parent entry with the wrong side bit", m_parent_side, 6), ("parent entry naming another node", m_parent_wrong, 6),
    ("slot_src entry duplicated", m_slot_src_dup, 5), ("8-wide qhi decremented", m_qhi_dec, 8), ("8-wide qlo incremented", m_qlo_inc, 8),
    ("8-wide box two steps loose", m_q_loose, 8), ("leaf_box shifted by one slot", m_leaf_box_shift, 8),
    ("4-wide box replaced by its parent's", m_box4_parent, 7), ("4-wide leaf ref to another leaf", m_ref4_wrong_leaf, 7),
    ("4-wide n_children short", m_nchildren4, 7), ("stack4 one short", m_stack4_short, 7), ("stack8 one short", m_stack8_short, 8),
    ("node row stale", m_row_stale_node, 9), ("triangle row stale", m_row_stale_tri, 9),
    ("4-wide row unit stale (ref)", m_row4_stale, 9), ("4-wide row unit stale (box)", m_row4_stale_box, 9),
    ("depth one short", m_depth_short, 10), ("scene bound off by one ulp", m_bounds, 10),
    ("edge off by one ulp", m_vertex, 5), ("normal off by one ulp", m_normal, 5),
]


@pytest.fixture(scope="module")
def flat_clean(built):
    snap, scene = host_snapshot(synth.soup(1000, 0.5, 1))
    assert not lc.check_flat(snap, scene.tris, leaf_boxes="host", nodes32=scene.nodes)
    return snap, scene


def _copy(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in snap.items()}


@pytest.mark.parametrize("name,mutate,rule", FLAT_MUTATIONS, ids=[m[0] for m in FLAT_MUTATIONS])
def test_flat_mutation_is_detected(flat_clean, name, mutate, rule):
    snap, scene = flat_clean
    bad = _copy(snap)
    mutate(bad)
    findings = lc.check_flat(bad, scene.tris, leaf_boxes="host", nodes32=scene.nodes)
    assert any(f.rule == rule for f in findings), f"{name}: not reported under rule {rule}\n{lc.summary(findings)}"
    print(f"{name}: detected by rule {rule} ({len(findings)} findings)")


def test_device_leaf_box_formula_has_teeth(flat_clean):
    """rule 3 in its device form (bounds of v0, v0 + e1, v0 + e2, one ulp outwards): a host tree's exact vertex boxes are not that
    formula's boxes, and boxes made by the formula pass; one face one ulp short of it is reported."""
    snap, scene = flat_clean
    assert any(f.rule == 3 for f in lc.check_flat(snap, scene.tris, leaf_boxes="device"))
    refit = _copy(snap)
    out = lc._Out()
    tree = lc.walk2(refit["nodes"], [0], 0, refit["n_nodes"], refit["n_tris"], out)
    mn, mx = lc.slot_boxes_device(refit["tri_hot"])
    lmn, lmx = lc._run_reduce(mn, tree.leaf_first, tree.leaf_count, np.minimum), lc._run_reduce(mx, tree.leaf_first, tree.leaf_count, np.maximum)
    for e, a, b in zip(tree.leaf_edges, lmn, lmx):
        side = "right" if e & 1 else "left"
        refit["nodes"][f"{side}_min"][tree.e_node[e]], refit["nodes"][f"{side}_max"][tree.e_node[e]] = a, b
    assert not [f for f in lc.check_flat(refit, scene.tris, leaf_boxes="device", skip=(2, 7, 8, 9, 10)) if f.rule == 3]
    assert lc.containment_slack(refit) == 0.0  # one ulp outwards of a sum rounded to nearest contains the float64 sum
    e = tree.leaf_edges[0]
    side = "right" if e & 1 else "left"
    refit["nodes"][f"{side}_max"][tree.e_node[e], 0] = _next(refit["nodes"][f"{side}_max"][tree.e_node[e], 0], False)
    assert any(f.rule == 3 for f in lc.check_flat(refit, scene.tris, leaf_boxes="device", skip=(2, 7, 8, 9, 10)))


def t_id_base(s):
    s["instances"]["id_base"][1] += 1


def t_inv_ulp(s):
    s["instances"]["inv"][2, 5] = _next(s["instances"]["inv"][2, 5], True)


def t_flag_cleared(s):
    s["instances"]["flags"][int(np.flatnonzero(s["instances"]["flags"] & 1)[0])] = 0


def t_index_dup(s):
    s["instances"]["index"][0] = s["instances"]["index"][1]


def t_layers(s):
    s["instances"]["layers"][3] ^= np.uint32(2)


def t_root(s):
    i = s["instances"]
    other = i["root"][i["root"] != i["root"][0]]
    i["root"][0] = other[0]


def t_tlas_leaf_box(s):
    nodes = s["nodes"]
    b = int(np.flatnonzero(nodes["left_idx"][:s["n_tlas_nodes"]] >= lc.LEAF)[0])
    nodes["left_max"][b, 0] = _next(nodes["left_max"][b, 0], False)


def t_tlas_nesting(s):
    nodes = s["nodes"]
    b = int(np.flatnonzero(nodes["left_idx"][:s["n_tlas_nodes"]] < lc.SENT)[0])  # (24 instances: the top level has inner nodes)
    nodes["left_min"][b, 1] = _next(nodes["left_min"][b, 1], False)


def t_blas_nesting(s):
    nodes, cap = s["nodes"], s["tlas_cap"]
    b = cap + int(np.flatnonzero(nodes["right_idx"][cap:] < lc.SENT)[0])
    nodes["right_max"][b, 2] = _next(nodes["right_max"][b, 2], False)


def t_blas_triangle(s):
    s["tri_hot"]["v0"][s["n_tris"] - 3, 1] = _next(s["tri_hot"]["v0"][s["n_tris"] - 3, 1], True)


TWO_LEVEL_MUTATIONS = [
    ("instance id_base off by one", t_id_base, 11), ("inverse transform element off by one ulp", t_inv_ulp, 12),
    ("TLAS leaf's last-instance flag cleared", t_flag_cleared, 1), ("registration index duplicated", t_index_dup, 11),
    ("instance layers changed", t_layers, 11), ("instance root of another mesh", t_root, 11),
    ("TLAS leaf box one ulp short", t_tlas_leaf_box, 12), ("TLAS inner box one ulp loose", t_tlas_nesting, 2),
    ("BLAS inner box one ulp short", t_blas_nesting, 2), ("BLAS triangle vertex off by one ulp", t_blas_triangle, 5),
]


@pytest.fixture(scope="module")
def two_level_clean(built):
    local, inst = synth.multi_mesh_instances(24, 100, 0.05, 11)
    inst["layers"] = 1 + np.arange(24) % 5
    snap = capi.two_level_prepare_host(local, inst)
    assert not lc.check_two_level(snap, local, inst, leaf_boxes="host")
    return snap, local, inst


@pytest.mark.parametrize("name,mutate,rule", TWO_LEVEL_MUTATIONS, ids=[m[0] for m in TWO_LEVEL_MUTATIONS])
def test_two_level_mutation_is_detected(two_level_clean, name, mutate, rule):
    snap, local, inst = two_level_clean
    bad = _copy(snap)
    mutate(bad)
    findings = lc.check_two_level(bad, local, inst, leaf_boxes="host")
    assert any(f.rule == rule for f in findings), f"{name}: not reported under rule {rule}\n{lc.summary(findings)}"
    print(f"{name}: detected by rule {rule} ({len(findings)} findings)")


def test_restated_formulas_on_edge_values():
    """ulp_down / ulp_up at zero, at the smallest normal and across signs, as the comment above them in refit.hip states"""
    f = np.array([0.0, -0.0, 1.0, -1.0, lc.FLT_MIN, -lc.FLT_MIN], dtype=np.float32)
    assert np.array_equal(lc.ulp_down(f), np.array([-lc.FLT_MIN, -lc.FLT_MIN, _next(1, False), _next(-1, False), _next(lc.FLT_MIN, False), _next(-lc.FLT_MIN, False)], dtype=np.float32))
    assert np.array_equal(lc.ulp_up(f), np.array([lc.FLT_MIN, lc.FLT_MIN, _next(1, True), _next(-1, True), _next(lc.FLT_MIN, True), _next(-lc.FLT_MIN, True)], dtype=np.float32))
    # world_box rounds outwards; invert_affine of a rotation + translation inverts it
    th = 0.3
    basis = np.array([[np.cos(th), -np.sin(th), 0, np.sin(th), np.cos(th), 0, 0, 0, 1]], dtype=np.float32)
    origin = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    lo, hi = lc.world_box(np.array([[-1, -1, -1]], np.float32), np.array([[1, 1, 1]], np.float32), basis, origin)
    B = basis.astype(np.float64).reshape(3, 3)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) @ B.T + origin.astype(np.float64)
    assert (lo.astype(np.float64) <= corners.min(axis=0)).all() and (hi.astype(np.float64) >= corners.max(axis=0)).all()
    inv = lc.invert_affine(basis, origin).reshape(3, 4).astype(np.float64)
    assert np.allclose(inv[:, :3] @ B, np.eye(3), atol=1e-6) and np.allclose(inv[:, :3] @ origin[0] + inv[:, 3], 0, atol=1e-6)
