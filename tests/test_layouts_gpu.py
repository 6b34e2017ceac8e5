"""Every resident acceleration layout against the CPU validator (tests/layout_check.py): after each call that produces or changes
a scene, Context.debug_snapshot copies the arrays out and the validator visits every node, child, slot and instance.  The
presence table below states which arrays a scene must have after which call; an array that is missing without the table's
condition is a failure.  Nothing here casts rays except the test that the snapshot is inert."""
import numpy as np
import pytest

import layout_check as lc
from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
from test_layouts_cpu import mixed_magnitudes, tiled_wall

pytestmark = pytest.mark.gpu

# Which arrays exist after which call, for a context made with KERNEL_AUTO and (the "quad" rows) with KERNEL_PACKET_QUAD; what the
# other kernel options keep resident (want4 / want8 / the rows depend on mrt_options.kernel) is not stated here.  From api.hip,
# refit.hip, tlas_device.hip:
#   every flat-scene path keeps nodes, triangles, the slot map, the 4-wide layout (AUTO wants it resident: want4 in
#   mrt_upload_scene / mrt_build_scene_device), the 8-wide layout with leaf_box, and the 64-byte row array; the parent table
#   appears with the first refit and stays; the 4-wide row array only in builds with the four-wide packet walk AND a context
#   that selects it.  A two-level scene keeps nodes, triangles, instance rows and the 8-wide BLAS layout; its slot map and
#   parent table appear with the first refit.  The one legitimate absence: nodes8 / leaf_box are dropped when a box fits no
#   grid (a non-finite extent; test_non_finite_box_drops_only_the_8_wide_layout).  A context that selects the four-wide packet
#   walk keeps the 4-wide layout and its row array, and neither the 8-wide layout nor the 64-byte rows.  A "device build" of one
#   triangle is a host upload (mrt_build_scene_device wraps the root leaf on the host): the same arrays.
ALWAYS_FLAT = {"nodes", "tri_hot", "tri_cold", "slot_src", "nodes4", "nodes8", "leaf_box", "rows"}
ALWAYS_TWO_LEVEL = {"nodes", "tri_hot", "tri_cold", "instances", "nodes8", "leaf_box"}
QUAD_FLAT = {"nodes", "tri_hot", "tri_cold", "slot_src", "nodes4", "rows4"}
PRESENCE = {
    ("flat", "upload"): ALWAYS_FLAT, ("flat", "build"): ALWAYS_FLAT, ("flat", "build1"): ALWAYS_FLAT, ("flat", "refit"): ALWAYS_FLAT | {"parent"},
    ("quad", "upload"): QUAD_FLAT, ("quad", "build"): QUAD_FLAT, ("quad", "refit"): QUAD_FLAT | {"parent"},
    ("two_level", "upload"): ALWAYS_TWO_LEVEL, ("two_level", "update"): ALWAYS_TWO_LEVEL,
    ("two_level", "refit"): ALWAYS_TWO_LEVEL | {"slot_src", "parent"},
}
NAMES = [name for name, _ in T.SNAPSHOT_ARRAYS]


def assert_presence(snap, kind, call, without=()):
    want = PRESENCE[(kind, call)] - set(without)
    have = {name for name in NAMES if snap[name] is not None}
    assert have == want, f"after {call} of a {kind} scene: arrays {sorted(have)}, expected {sorted(want)}"


SLACK = {}  # rule 4 figures of this run, printed by the tests: what -> (ulp on this tree, ulp on the host tree of the same triangles)


def host_slack(tris, verts9):
    """rule 4's baseline: the worst containment slack on the host-built tree of these triangles (the arrays an upload would upload)"""
    nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts9))
    return lc.containment_slack(capi.prepare_scene_host(tris, nodes, prim_idx))


def assert_slack(snap, baseline, what):
    slack = lc.containment_slack(snap)
    SLACK[what] = (slack, baseline)
    assert slack <= baseline, f"rule 4, {what}: a vertex lies {slack:.6g} ulp outside its leaf box; on the host tree of the same triangles {baseline:.6g}"
    return slack


def check_flat(c, tris, call, leaf_boxes="device", nodes32=None, what="", kind="flat", verts=None):
    """snapshot, presence, every rule; with verts (the vertices tris were made from) also rule 4 against the host tree"""
    snap = c.debug_snapshot()
    # (the 4-wide rows exist only while the 4-wide walk's worst-case stack fits the wave's 64 entries: build_rows in api.hip)
    assert_presence(snap, kind, call, without=("rows4",) if kind == "quad" and snap["stack4"] > 64 else ())
    assert snap["two_level"] == 0 and snap["n_tris"] == tris.shape[0] and snap["n_instances"] == 0
    findings = lc.check_flat(snap, tris, leaf_boxes=leaf_boxes, nodes32=nodes32)
    assert not findings, f"{what} after {call}:\n{lc.summary(findings)}"
    assert c.scene_info()["stack_need"] == snap["depth"]
    if verts is not None:
        assert_slack(snap, host_slack(tris, verts), f"{what} after {call}")
    return snap


FORMS = {"radix": {}, "radix_safe": {"safe_handoff": True}, "ploc": {"ploc": True}, "sah": {"sah": True}}


def degenerate():
    same = np.repeat(synth.soup(1, 0.5, 3), 300, axis=0)
    return np.concatenate([same, synth.soup(50, 0.2, 4) * 0.001, synth.soup(1, 0.5, 9) + 4.0]).astype(np.float32)


FLAT_SCENES = {
    "soup1": lambda: synth.soup(1, 2.0, 5), "soup2": lambda: synth.soup(2, 2.0, 6), "soup3": lambda: synth.soup(3, 1.5, 7),
    "soup17": lambda: synth.soup(17, 1.0, 8), "soup33": lambda: synth.soup(33, 1.0, 9), "soup1000": lambda: synth.soup(1000, 0.5, 1),
    "soup20000": lambda: synth.soup(20000, 0.25, 33), "degenerate": degenerate, "wall": tiled_wall,
    "room": lambda: synth.flatten_instances(*synth.room()), "mixed": mixed_magnitudes,
}


@pytest.mark.parametrize("name", list(FLAT_SCENES))
def test_flat_paths(built, name):
    """Host upload and every device build form, each followed by: a refit (derives the parent table; a host tree's wide layouts
    move to binary-node indices), a second refit (reuses them), and a refit back to the first vertices.  Rule 4: no device-made
    box lets a vertex lie further outside than the host tree of the same triangles does."""
    v = FLAT_SCENES[name]()
    n = v.shape[0]
    ids = np.arange(n, dtype=np.uint32)[::-1].copy()
    layers = (1 << (np.arange(n) % 3)).astype(np.uint32)
    tris = capi.make_triangles(v, ids, layers)
    scene = capi.Scene(v)
    c = capi.Context(0)
    slack = {}
    try:
        for source in ["host"] + list(FORMS):
            if source == "host":
                c.upload_scene(tris, scene.nodes, scene.prim_idx)
                snap = check_flat(c, tris, "upload", "host", scene.nodes, f"{name} host")
                slack["host"] = lc.containment_slack(snap)
            else:
                c.build_scene_device(tris, **FORMS[source])
                # (one triangle has no device tree: mrt_build_scene_device takes the host path, whose boxes are the exact bounds)
                snap = check_flat(c, tris, "build" if n > 1 else "build1", "device" if n > 1 else "host",
                                  capi.bvh2_build(T.verts4_from_verts9(v))[0] if n == 1 else None, f"{name} {source}")
                slack[source] = lc.containment_slack(snap)
            for k, (amp, phase) in enumerate(((0.3, 0.9), (0.05, 2.1), (0.0, 0.0))):
                v1 = synth.deform(v, amp, phase, 3)
                tris1 = capi.make_triangles(v1, ids if k != 1 else None, layers)
                c.refit_scene(tris1)
                # (the refit's triangles have their own host tree: the baseline is measured on it)
                snap = check_flat(c, tris1, "refit", what=f"{name} {source} refit {k}", verts=v1)
                slack[f"{source}+refit{k}"] = lc.containment_slack(snap)
    finally:
        c.close()
    print(f"rule 4, {name}: " + ", ".join(f"{k} {s:.3g}" for k, s in slack.items()))
    worst = max((s, k) for k, s in slack.items() if k != "host" and "refit" not in k)
    assert worst[0] <= slack["host"], f"{name}: vertices up to {worst[0]:.3g} ulp outside their leaf box after {worst[1]}; host tree {slack['host']:.3g}"


@pytest.mark.parametrize("path", ["host", "radix"])
def test_large_soup(built, path):
    """100 000 triangles: the compact host layouts, and the binary-index layouts of a device build and a refit"""
    v = synth.soup(100000, 0.12, 77)
    tris = capi.make_triangles(v)
    c = capi.Context(0)
    try:
        if path == "host":
            scene = capi.Scene(v)
            c.upload_scene(tris, scene.nodes, scene.prim_idx)
            check_flat(c, tris, "upload", "host", scene.nodes, "soup100000 host", verts=v)
        else:
            c.build_scene_device(tris)
            check_flat(c, tris, "build", what="soup100000 radix", verts=v)
            v1 = synth.deform(v, 0.1, 0.4, 3)
            tris1 = capi.make_triangles(v1)
            c.refit_scene(tris1)
            check_flat(c, tris1, "refit", what="soup100000 radix refit", verts=v1)
        print("rule 4: " + ", ".join(f"{k} {a:.3g} (host {b:.3g})" for k, (a, b) in SLACK.items() if k.startswith("soup100000")))
    finally:
        c.close()


def test_motions_that_would_show_a_stale_box(built):
    """A mesh grown past its old box, shuffled vertices, triangles collapsed to points, on a host tree and a device tree: a box
    kept from before the motion is too small or too large for the new triangles, and rules 2 and 3 say so."""
    v = synth.soup(5000, 0.3, 12)
    for source in ("host", "ploc"):
        c = capi.Context(0)
        try:
            tris = capi.make_triangles(v)
            if source == "host":
                capi.Scene(v).upload(c)
            else:
                c.build_scene_device(tris, ploc=True)
            grown = (v * np.float32(3.0) + np.float32(1.5)).astype(np.float32)
            shuffled = v[np.random.default_rng(5).permutation(v.shape[0])]
            points = v.copy()
            points[::2] = v[::2].mean(axis=1, keepdims=True)
            for what, frame in (("grown", grown), ("shuffled", shuffled), ("half points", points), ("back", v)):
                t1 = capi.make_triangles(frame)
                c.refit_scene(t1)
                check_flat(c, t1, "refit", what=f"{source} {what}", verts=frame)
        finally:
            c.close()


def test_sequences_in_one_context(built):
    """One context through: a small device build, a larger one (the arena grows), every form after another, triangles already on
    the device, a host upload after a device build and the reverse, an instanced build and its refit."""
    c = capi.Context(0)
    try:
        small, large = synth.soup(500, 0.5, 2), synth.soup(30000, 0.2, 3)
        for v, kw in ((small, {}), (large, {}), (large, {"sah": True}), (small, {"ploc": True}), (large, {"ploc": True}), (small, {"sah": True}), (large, {"safe_handoff": True})):
            tris = capi.make_triangles(v)
            c.build_scene_device(tris, **kw)
            check_flat(c, tris, "build", what=f"{v.shape[0]} {kw}", verts=v)
        tris = capi.make_triangles(small)
        d = c.device_alloc(tris.nbytes)
        c.h2d(d, tris)
        c.build_scene_device(d, n_tris=tris.shape[0], on_device=True)
        check_flat(c, tris, "build", what="triangles on the device", verts=small)
        small1 = synth.deform(small, 0.2, 1.0, 4)
        tris1 = capi.make_triangles(small1)
        c.h2d(d, tris1)
        c.refit_scene(d, n_tris=tris1.shape[0], on_device=True)
        check_flat(c, tris1, "refit", what="refit from the device", verts=small1)
        c.device_free(d)
        scene = capi.Scene(large)
        c.upload_scene(scene.tris, scene.nodes, scene.prim_idx)          # a host upload drops the parent table of the scene before
        check_flat(c, scene.tris, "upload", "host", scene.nodes, "host after device")
        c.build_scene_device(scene.tris)
        check_flat(c, scene.tris, "build", what="device after host", verts=large)
        local, inst = synth.multi_mesh_instances(5, 300, 0.05, 11)
        inst["layers"] = [1, 2, 4, 8, 16]
        c.build_instanced_scene_device(local, inst)
        check_flat(c, po.flatten_instances(local, inst), "build", what="instanced build", verts=synth.flatten_instances(local, inst))
        moved = inst.copy()
        moved["origin"] += np.float32(0.25)
        local1 = synth.deform(local, 0.02, 0.7, 2)
        c.refit_instanced_scene(local1, moved)
        check_flat(c, po.flatten_instances(local1, moved), "refit", what="instanced refit", verts=synth.flatten_instances(local1, moved))
    finally:
        c.close()


@pytest.mark.skipif(not capi.kernel_available(capi.KERNEL_PACKET_QUAD), reason="built without MRT_WITH_QUAD")
@pytest.mark.parametrize("source", ["host", "radix", "sah"])
def test_four_wide_row_array(built, source):
    """A context that selects the four-wide packet walk keeps the 4-wide layout and its row array (rule 9: rebuilt from the
    snapshot's 4-wide nodes and triangles, byte for byte).  A host tree's first refit moves the 4-wide layout from its compact form
    to binary-node indices and re-sizes the row array with it; the second refit rewrites both in place."""
    v = synth.soup(3000, 0.35, 17)
    tris = capi.make_triangles(v)
    c = capi.Context(0, kernel=capi.KERNEL_PACKET_QUAD)
    try:
        if source == "host":
            scene = capi.Scene(v)
            c.upload_scene(tris, scene.nodes, scene.prim_idx)
            compact = check_flat(c, tris, "upload", "host", scene.nodes, "quad host", kind="quad", verts=v)
        else:
            c.build_scene_device(tris, sah=source == "sah")
            check_flat(c, tris, "build", what=f"quad {source}", kind="quad", verts=v)
        for k, phase in enumerate((0.4, 2.1)):
            v1 = synth.deform(v, 0.1, phase, 3)
            tris1 = capi.make_triangles(v1)
            c.refit_scene(tris1)
            snap = check_flat(c, tris1, "refit", what=f"quad {source} refit {k}", kind="quad", verts=v1)
            assert snap["n_nodes4"] == snap["n_nodes"]
            assert source == "radix" or snap["rows4"] is not None, "a SAH tree of 3000 triangles is far shallower than 21 levels"
            assert snap["rows4"] is None or snap["rows4"].shape[0] == 2 * snap["n_nodes"] + snap["n_tris"]
        if source == "host":
            assert compact["n_nodes4"] < compact["n_nodes"]
    finally:
        c.close()


def test_non_finite_box_drops_only_the_8_wide_layout(built):
    """The presence table's one condition: a box that fits no 8-bit grid.  The caller's boxes are the caller's: a leaf box whose
    upper face is at +inf is a valid (loose) BVH, its extent is not finite, and the scene goes without nodes8 / leaf_box -- and
    without nothing else; every other rule still holds on it."""
    v = synth.soup(200, 0.5, 21)
    scene = capi.Scene(v)
    nodes = scene.nodes.copy()
    path = [0]                                   # the root and its rightmost descendants, down to a leaf, open upwards in x
    while nodes["tri_count"][path[-1]] == 0:
        path.append(int(nodes["left_first"][path[-1]]) + 1)
    nodes["aabb_max"][path, 0] = np.inf
    c = capi.Context(0)
    try:
        c.upload_scene(scene.tris, nodes, scene.prim_idx)
        snap = c.debug_snapshot()
        assert_presence(snap, "flat", "upload", without=("nodes8", "leaf_box"))
        assert snap["n_nodes8"] == 0 and snap["stack8"] == 0
        findings = lc.check_flat(snap, scene.tris, leaf_boxes="host", nodes32=nodes)
        assert not findings, lc.summary(findings)
    finally:
        c.close()


# ---- two-level scenes ------------------------------------------------------------------------------------------------------------

def check_two_level(c, local, inst, call, leaf_boxes, what="", baseline=None):
    """snapshot, presence, every rule; baseline: rule 4's figure on the host-built BLASes of the same mesh vertices"""
    snap = c.debug_snapshot()
    assert_presence(snap, "two_level", call)
    assert snap["two_level"] == 1 and snap["n_instances"] == inst.shape[0] and snap["n_nodes4"] == 0
    findings = lc.check_two_level(snap, local, inst, leaf_boxes=leaf_boxes)
    assert not findings, f"{what} after {call}:\n{lc.summary(findings)}"
    if baseline is not None:
        assert_slack(snap, baseline, f"{what} after {call}")
    return snap


def host_slack_two_level(local, inst):
    return lc.containment_slack(capi.two_level_prepare_host(local, inst))


def multi8():
    """eight meshes, two of them placed twice"""
    local, inst = synth.multi_mesh_instances(8, 2000, 0.05, 11)
    extra = inst[[1, 5]].copy()
    extra["origin"] += np.float32(0.7)
    inst = np.concatenate([inst, extra])
    inst["layers"] = 1 << (np.arange(inst.shape[0]) % 4)
    return local, inst


def moved_instances(inst, k):
    out = inst.copy()
    out["origin"] += np.float32(0.1 * (k + 1))
    a = np.float32(0.3 * (k + 1))
    turn = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    out["basis"] = (turn @ inst["basis"].reshape(-1, 3, 3)).astype(np.float32).reshape(-1, 9)
    out["layers"] = np.roll(inst["layers"], k + 1)
    return out


TWO_LEVEL_SCENES = {"room": synth.room, "multi8": multi8, "many65536": lambda: synth.many_instances(65536),
                    "one": lambda: synth.multi_mesh_instances(1, 200, 0.05, 5)}
UPLOADS = {"host": ({}, "host"), "device": ({"blas_on_device": True}, "device"), "device_sah": ({"blas_on_device": True, "sah": True}, "device")}


@pytest.mark.parametrize("upload", list(UPLOADS))
@pytest.mark.parametrize("name", list(TWO_LEVEL_SCENES))
def test_two_level_paths(built, name, upload):
    """Upload (host BLASes, device BLASes, device SAH), then: update on the host; update on the device in each form from a host and
    from a device instance array; a refit of the meshes (makes the slot map and the parent table, moves a host scene's 8-wide
    layout to binary indices, and leaves the device top level's mesh table stale); updates again, which must box the instances by
    the refit meshes; a refit with the instances on the device."""
    local, inst = TWO_LEVEL_SCENES[name]()
    kw, boxes = UPLOADS[upload]
    c = capi.Context(0)
    d_inst = c.device_alloc(inst.nbytes)
    try:
        base = host_slack_two_level(local, inst)
        c.upload_two_level_scene(local, inst, **kw)
        check_two_level(c, local, inst, "upload", boxes, f"{name} {upload}", base)
        step = 0

        def updates(verts, call, leaf_boxes, base):
            nonlocal step
            cur = moved_instances(inst, step); step += 1
            c.update_instances(cur)
            check_two_level(c, verts, cur, call, leaf_boxes, f"{name} {upload} host update", base)
            for form in capi.TLAS_FORMS:
                for on_device in (False, True):
                    cur = moved_instances(inst, step); step += 1
                    if on_device:
                        c.h2d(d_inst, cur)
                    c.update_instances_device(d_inst if on_device else cur, on_device=on_device, form=form, n_instances=cur.shape[0])
                    check_two_level(c, verts, cur, call, leaf_boxes, f"{name} {upload} device update {form} on_device={on_device}", base)

        updates(local, "update", boxes, base)
        local1 = synth.deform(local, 0.05, 0.8, 2)
        base1 = host_slack_two_level(local1, inst)
        cur = moved_instances(inst, 20)
        c.refit_two_level_scene(local1, cur)
        check_two_level(c, local1, cur, "refit", "device", f"{name} {upload} refit", base1)
        updates(local1, "refit", "device", base1)
        local2 = (local * np.float32(1.5)).astype(np.float32)          # every mesh grown past its old box
        base2 = host_slack_two_level(local2, inst)
        cur = moved_instances(inst, 21)
        c.h2d(d_inst, cur)
        c.refit_two_level_scene(local2, d_inst, instances_on_device=True, n_instances=cur.shape[0])
        check_two_level(c, local2, cur, "refit", "device", f"{name} {upload} refit with device instances", base2)
        c.update_instances(inst)
        check_two_level(c, local2, inst, "refit", "device", f"{name} {upload} host update after the device refit", base2)
        worst = max(SLACK[k] for k in SLACK if k.startswith(f"{name} {upload}"))
        print(f"rule 4, {name} {upload}: worst {worst[0]:.3g} ulp (host BLASes: {base:.3g}, {base1:.3g}, {base2:.3g})")
    finally:
        c.device_free(d_inst)
        c.close()


def test_a_scene_of_the_other_kind_replaces_every_array(built):
    """flat -> two-level -> flat in one context: the snapshot reports exactly the new scene's arrays"""
    v = synth.soup(2000, 0.4, 9)
    tris = capi.make_triangles(v)
    local, inst = synth.room()
    c = capi.Context(0)
    try:
        c.build_scene_device(tris)
        c.refit_scene(tris)
        check_flat(c, tris, "refit", what="flat")
        c.upload_two_level_scene(local, inst)
        check_two_level(c, local, inst, "upload", "host", "two-level after flat")
        c.refit_two_level_scene(local, inst)
        check_two_level(c, local, inst, "refit", "device", "two-level refit")
        scene = capi.Scene(v)
        c.upload_scene(scene.tris, scene.nodes, scene.prim_idx)
        check_flat(c, scene.tris, "upload", "host", scene.nodes, "flat after two-level")
        c.upload_two_level_scene(local, inst, blas_on_device=True)
        check_two_level(c, local, inst, "upload", "device", "two-level after flat again")
        c.build_scene_device(tris, sah=True)
        check_flat(c, tris, "build", what="flat again")
    finally:
        c.close()


def test_the_snapshot_is_inert(built):
    """A grid cast and an incoherent batch, a snapshot, the same casts again: the same bytes from the same kernels.  Two snapshots in
    a row are equal.  Between submit and collect the snapshot is refused (MRT_ERR_PENDING), without a scene MRT_ERR_NO_SCENE."""
    v = synth.soup(20000, 0.25, 33)
    c = capi.Context(0)
    try:
        with pytest.raises(capi.MrtError) as e:
            c.debug_snapshot()
        assert e.value.status == capi.ERR_NO_SCENE
        capi.Scene(v).upload(c)
        cam = capi.camera_look((0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 512, 512, 50.0)
        rays = synth.incoherent_rays(100000, 11)

        def casts():
            out = []
            for _ in range(3):  # (the grid tuner and the tile schedule settle over repeated casts of one grid)
                grid = c.cast_grid(cam, 512, 512)
                out.append((grid.tobytes(), c.last_kernel_variant()))
            inc = c.cast(rays)
            out.append((inc.tobytes(), c.last_kernel_variant()))
            return out

        before = casts()
        for _ in range(8):  # until the context has settled on its kernels for these batches
            again = casts()
            settled, before = [x[1] for x in again] == [x[1] for x in before], again
            if settled:
                break
        assert settled, "the casts' kernel choice did not settle"
        stats = c.stats()
        a = c.debug_snapshot()
        b = c.debug_snapshot()
        assert c.stats() == stats and not c.has_pending()
        for name in NAMES:
            assert (a[name] is None) == (b[name] is None) and (a[name] is None or a[name].tobytes() == b[name].tobytes()), name
        after = casts()
        assert [x[1] for x in before] == [x[1] for x in after] and [x[0] for x in before] == [x[0] for x in after]
        c.submit(rays)
        with pytest.raises(capi.MrtError) as e:
            c.debug_snapshot()
        assert e.value.status == capi.ERR_PENDING and c.has_pending()
        hits = c.collect()
        assert hits.tobytes() == after[-1][0]
        assert c.debug_snapshot(arrays=False)["n_tris"] == 20000
    finally:
        c.close()
