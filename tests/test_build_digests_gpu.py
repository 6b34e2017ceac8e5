"""The bytes the scene builders write, pinned: sha256 of every mrt_debug_snapshot array after each path that makes or changes a
scene, against tests/golden/build_digests.json (recorded by tests/golden/make_build_digests.py on the commit before the
builders' rules moved into csrc/build_rules.h).  The oracle tests hold hits and layout_check.py holds validity within a looseness
bound; this holds "the same arrays".  The builders are deterministic (device_build.hip: ranks, rows and leaf order do not depend
on the creation order of nodes), so a digest that moves is a rule that moved.

A digest covers the elements the scene defines, and nothing a builder leaves unwritten:
  * flat scenes: every row of every array; leaf_box only at each leaf's first slot (device builds write no other);
  * two-level scenes: the TLAS rows [0, n_tlas_nodes) and the BLAS rows reached from the instances' roots (the rows between
    tlas_cap and a BLAS, and behind a device SAH BLAS that fills fewer than n_tris - 1, are nobody's); parent and a binary-index
    8-wide layout at the same rows;
  * padding fields are left out; the scalars (counts, depth, stack bounds, bounds) are digested as one more entry."""
import hashlib
import json
import os

import numpy as np
import pytest

import layout_check as lc
from messyerraytracer_amd import capi, synth, types as T
from test_layouts_cpu import two_level_inputs
from test_layouts_gpu import moved_instances

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_digests.json")
SCALARS = ["two_level", "n_nodes", "n_tris", "n_nodes4", "n_nodes8", "depth", "stack_depth", "stack4", "stack8", "n_tlas_nodes",
           "tlas_cap", "n_instances"]


def _sha(a, rows=None):
    """sha256 over rows (all if None) of an array; a structured array field by field, fields named pad left out"""
    h = hashlib.sha256()
    if rows is not None:
        a = a[rows]
    if a.dtype.names:
        for name in a.dtype.names:
            if name != "pad":
                h.update(np.ascontiguousarray(a[name]).tobytes())
    else:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests(snap):
    """name -> sha256 of the defined elements of every array of a snapshot, and of its scalars"""
    out = {"scalars": hashlib.sha256(json.dumps(
        [int(snap[k]) for k in SCALARS] + [int(x) for x in np.concatenate([snap["bounds_lo"], snap["bounds_hi"], [snap["scene_abs_max"]]])
                                           .astype(np.float32).view(np.uint32)]).encode()).hexdigest()}
    nodes, n_tris = snap["nodes"], snap["tri_hot"].shape[0]
    findings = lc._Out()
    if snap["two_level"]:
        cap = int(snap["tlas_cap"])
        roots = np.unique(snap["instances"]["root"]).astype(np.int64)
        t = lc.walk2(nodes, roots, cap, nodes.shape[0], n_tris, findings, wrapped_ok=False)
        blas_rows = np.sort(t.order)
        node_rows = np.concatenate([np.arange(int(snap["n_tlas_nodes"])), blas_rows])
        binary8 = snap["nodes8"] is not None and snap["nodes8"].shape[0] == nodes.shape[0] - cap and \
            bool((snap["instances"]["root8"].astype(np.int64) == snap["instances"]["root"].astype(np.int64) - cap).all())
        rows_of = {"nodes": node_rows, "parent": blas_rows - cap, "nodes8": blas_rows - cap if binary8 else None}
    else:
        t = lc.walk2(nodes, [0], 0, nodes.shape[0], n_tris, findings, cover=True)
        rows_of = {}
    assert not findings, lc.summary(list(findings))
    rows_of["leaf_box"] = t.leaf_first
    for name, _ in T.SNAPSHOT_ARRAYS:
        if snap[name] is not None:
            out[name] = _sha(snap[name], rows_of.get(name))
    return out


# ---- the cases: group -> {case: digests}; a group is one context ------------------------------------------------------------------

SOUPS = {"soup2": (2, 2.0, 6), "soup3": (3, 1.5, 7), "soup17": (17, 1.0, 8), "soup1000": (1000, 0.5, 1)}  # test_device_build_gpu.py
FLAT_PATHS = {"host": None, "radix": {}, "ploc": {"ploc": True}, "sah": {"sah": True}}
UPLOADS = {"host": {}, "device": {"blas_on_device": True}, "device_sah": {"blas_on_device": True, "sah": True}}


def degenerate():
    """test_degenerate_inputs_for_the_device_builders: 300 coincident triangles, a flat cluster, an outlier; ids reversed"""
    same = np.repeat(synth.soup(1, 0.5, 3), 300, axis=0)
    v = np.concatenate([same, synth.soup(50, 0.2, 4) * 0.001, synth.soup(1, 0.5, 9) + 4.0]).astype(np.float32)
    return v, np.arange(v.shape[0], dtype=np.uint32)[::-1].copy()


def flat_group(name, path):
    if name in SOUPS:
        v = synth.soup(*SOUPS[name])
        ids, layers = None, (1 << (np.arange(v.shape[0]) % 3)).astype(np.uint32)
    elif name == "degenerate":
        (v, ids), layers = degenerate(), None
    else:  # the 300 coincident triangles alone: no plane separates them, the SAH root stays a leaf and is wrapped
        v, ids, layers = np.repeat(synth.soup(1, 0.5, 3), 300, axis=0), None, None
    tris = capi.make_triangles(v, ids, layers)
    out = {}
    c = capi.Context(0)
    try:
        if path == "host":
            scene = capi.Scene(v)
            c.upload_scene(tris, scene.nodes, scene.prim_idx)
        else:
            c.build_scene_device(tris, **FLAT_PATHS[path])
        out[f"{name}/{path}"] = digests(c.debug_snapshot())
        if name in SOUPS:
            c.refit_scene(capi.make_triangles(synth.deform(v, 0.3, 0.9, 3), ids, layers))
            out[f"{name}/{path}+refit"] = digests(c.debug_snapshot())
    finally:
        c.close()
    return out


def two_level_group(name, upload):
    local, inst = two_level_inputs(name)
    out = {}
    c = capi.Context(0)
    try:
        c.upload_two_level_scene(local, inst, **UPLOADS[upload])
        out[f"{name}/{upload}"] = digests(c.debug_snapshot())
        c.refit_two_level_scene(synth.deform(local, 0.05, 0.8, 2), moved_instances(inst, 20))
        out[f"{name}/{upload}+refit"] = digests(c.debug_snapshot())
        for k, form in enumerate(capi.TLAS_FORMS):
            c.update_instances_device(moved_instances(inst, k), form=form)
            out[f"{name}/{upload}+refit+update_{form}"] = digests(c.debug_snapshot())
    finally:
        c.close()
    return out


GROUPS = {f"{name}-{path}": (flat_group, name, path) for name in SOUPS for path in FLAT_PATHS}
GROUPS.update({"degenerate-sah": (flat_group, "degenerate", "sah"), "coincident300-sah": (flat_group, "coincident300", "sah")})
GROUPS.update({f"{name}-{upload}": (two_level_group, name, upload) for name in ("room", "multi4") for upload in UPLOADS})


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("group", list(GROUPS))
def test_builders_write_the_recorded_bytes(built, recorded, group):
    fn, name, path = GROUPS[group]
    got = fn(name, path)
    differ = []
    for case, have in got.items():
        assert case in recorded["digests"], f"{case} is not in the fixture"
        want = recorded["digests"][case]
        left_out = set(recorded["unstable"].get(case, []))  # arrays two recordings of the parent disagreed on (none: see the fixture)
        assert set(have) - left_out == set(want), f"{case}: arrays {sorted(have)}, recorded {sorted(want)}"
        differ += [f"{case}: {a}" for a in want if have[a] != want[a]]
    assert not differ, "arrays that are not the recorded bytes:\n" + "\n".join(differ)
