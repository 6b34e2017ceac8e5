"""Which instantiation a primary cast runs, by its exact name (mrt_last_kernel_variant), for every forced kernel option and
MRT_KERNEL_AUTO: a 64x64 grid made in the kernel (mrt_cast_grid) and the same 4 096 rays from an array, declared coherent and not
(mrt_cast), closest hit and any hit, with and without visit counters, on synth.room() flat and as a two-level scene; for the 128-ray
walk also both workgroup sizes and culling on and off.  Every cast is held to the oracle as well.  The names are the ones these casts
reported before the launch was resolved in launch_policy.cpp (resolve_trace / resolve_persistent): the table below was printed by this
file's own casts at that commit."""
import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
import parity

pytestmark = pytest.mark.gpu

W = H = 64
ORIGIN, FWD, FOV = (0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0
KERNELS = {"LANE": capi.KERNEL_LANE, "PACKET": capi.KERNEL_PACKET, "PACKET_ASM": capi.KERNEL_PACKET_ASM,
           "PACKET_ROWS": capi.KERNEL_PACKET_ROWS, "PACKET_DUAL": capi.KERNEL_PACKET_DUAL,
           "LANE_PERSISTENT": capi.KERNEL_LANE_PERSISTENT, "LANE4_PERSISTENT": capi.KERNEL_LANE4_PERSISTENT,
           "LANE8_PERSISTENT": capi.KERNEL_LANE8_PERSISTENT, "AUTO": capi.KERNEL_AUTO}
CASTS = ("grid", "coherent", "plain")  # mrt_cast_grid; mrt_cast with FLAG_COHERENT; mrt_cast without

# (scene, kernel option, count_visits) -> the name after each of CASTS; {A} = "true" in any-hit mode, "false" in closest-hit mode
EXPECT = {
    ('room', 'LANE', 0): ('trace_lane_kernel<{A}, false>', 'trace_lane_kernel<{A}, false>', 'trace_lane_kernel<{A}, false>'),
    ('room', 'LANE', 1): ('trace_lane_kernel<{A}, true>', 'trace_lane_kernel<{A}, true>', 'trace_lane_kernel<{A}, true>'),
    ('room', 'PACKET', 0): (
        'trace_packet_kernel<{A}, false>', 'trace_packet_kernel<{A}, false>',
        'trace_packet_kernel<{A}, false>'),
    ('room', 'PACKET', 1): ('trace_packet_kernel<{A}, true>', 'trace_packet_kernel<{A}, true>', 'trace_packet_kernel<{A}, true>'),
    ('room', 'PACKET_ASM', 0): (
        'trace_packet_asm_kernel<{A}, false, true>', 'trace_packet_asm_kernel<{A}, false, true>',
        'trace_packet_asm_kernel<{A}, false, true>'),
    ('room', 'PACKET_ASM', 1): (
        'trace_packet_asm_kernel<{A}, true>', 'trace_packet_asm_kernel<{A}, true>',
        'trace_packet_asm_kernel<{A}, true>'),
    ('room', 'PACKET_ROWS', 0): (
        'trace_packet_rows_kernel<{A}, false, 1, 256, false>', 'trace_packet_rows_kernel<{A}, false, 1, 256, false>',
        'trace_lane_kernel<{A}, false>'),
    ('room', 'PACKET_ROWS', 1): (
        'trace_packet_rows_kernel<{A}, true, 1, 256, false>', 'trace_packet_rows_kernel<{A}, true, 1, 256, false>',
        'trace_lane_kernel<{A}, true>'),
    ('room', 'PACKET_DUAL', 0): (
        'trace_packet_rows_kernel<{A}, false, 2, 64, true>', 'trace_packet_rows_kernel<{A}, false, 2, 64, false>',
        'trace_lane_kernel<{A}, false>'),
    ('room', 'PACKET_DUAL', 1): (
        'trace_packet_rows_kernel<{A}, true, 2, 64, true>', 'trace_packet_rows_kernel<{A}, true, 2, 64, false>',
        'trace_lane_kernel<{A}, true>'),
    ('room', 'LANE_PERSISTENT', 0): (
        'trace_lane_kernel<{A}, false>', 'trace_lane_persistent_kernel<{A}, 2, false, false>',
        'trace_lane_persistent_kernel<{A}, 2, false, false>'),
    ('room', 'LANE_PERSISTENT', 1): (
        'trace_lane_kernel<{A}, true>', 'trace_lane_persistent_kernel<{A}, 2, false, true>',
        'trace_lane_persistent_kernel<{A}, 2, false, true>'),
    ('room', 'LANE4_PERSISTENT', 0): (
        'trace_lane_kernel<{A}, false>', 'trace_lane_persistent_kernel<{A}, 4, false, false>',
        'trace_lane_persistent_kernel<{A}, 4, false, false>'),
    ('room', 'LANE4_PERSISTENT', 1): (
        'trace_lane_kernel<{A}, true>', 'trace_lane_persistent_kernel<{A}, 4, false, true>',
        'trace_lane_persistent_kernel<{A}, 4, false, true>'),
    ('room', 'LANE8_PERSISTENT', 0): (
        'trace_lane_kernel<{A}, false>', 'trace_lane_persistent_kernel<{A}, 8, false, false>',
        'trace_lane_persistent_kernel<{A}, 8, false, false>'),
    ('room', 'LANE8_PERSISTENT', 1): (
        'trace_lane_kernel<{A}, true>', 'trace_lane_persistent_kernel<{A}, 8, false, true>',
        'trace_lane_persistent_kernel<{A}, 8, false, true>'),
    ('room', 'AUTO', 0): (
        'trace_packet_asm_kernel<{A}, false, true>', 'trace_packet_asm_kernel<{A}, false, true>',
        'trace_lane_kernel<{A}, false>'),
    ('room', 'AUTO', 1): ('trace_lane_kernel<{A}, true>', 'trace_lane_kernel<{A}, true>', 'trace_lane_kernel<{A}, true>'),
    ('room_tl', 'LANE', 0): ('trace_two_level_kernel<{A}>', 'trace_two_level_kernel<{A}>', 'trace_two_level_kernel<{A}>'),
    ('room_tl', 'LANE', 1): ('trace_two_level_kernel<{A}>', 'trace_two_level_kernel<{A}>', 'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET', 1): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET_ASM', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET_ASM', 1): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET_ROWS', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET_ROWS', 1): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET_DUAL', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'PACKET_DUAL', 1): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'LANE_PERSISTENT', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'LANE_PERSISTENT', 1): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'LANE4_PERSISTENT', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'LANE4_PERSISTENT', 1): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'LANE8_PERSISTENT', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_lane_persistent_kernel<{A}, 8, true, false>'),
    ('room_tl', 'LANE8_PERSISTENT', 1): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'AUTO', 0): (
        'trace_two_level_packet_kernel<{A}>', 'trace_two_level_packet_kernel<{A}>',
        'trace_two_level_kernel<{A}>'),
    ('room_tl', 'AUTO', 1): ('trace_two_level_kernel<{A}>', 'trace_two_level_kernel<{A}>', 'trace_two_level_kernel<{A}>'),
}
# the 128-ray walk: (packet_wg, packet_cull) -> the same three
EXPECT_DUAL = {
    (64, 1): (
        'trace_packet_rows_kernel<{A}, false, 2, 64, false>', 'trace_packet_rows_kernel<{A}, false, 2, 64, false>',
        'trace_lane_kernel<{A}, false>'),
    (64, 2): (
        'trace_packet_rows_kernel<{A}, false, 2, 64, true>', 'trace_packet_rows_kernel<{A}, false, 2, 64, true>',
        'trace_lane_kernel<{A}, false>'),
    (256, 1): (
        'trace_packet_rows_kernel<{A}, false, 2, 256, false>', 'trace_packet_rows_kernel<{A}, false, 2, 256, false>',
        'trace_lane_kernel<{A}, false>'),
    (256, 2): (
        'trace_packet_rows_kernel<{A}, false, 2, 256, true>', 'trace_packet_rows_kernel<{A}, false, 2, 256, true>',
        'trace_lane_kernel<{A}, false>'),
}


def make_room():
    """synth.room() flat and two-level, the 4 096 rays and what the oracle says of them in each scene"""
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    rays = po.grid_rays(ORIGIN, FWD, W, H, FOV)
    want = {"room": po.OracleScene(verts, layers=layers).trace(rays), "room_tl": po.OracleTwoLevelScene(local, inst).trace(rays)}
    assert (want["room"]["prim_id"] >= 0).any()
    return dict(local=local, inst=inst, verts=verts, layers=layers, rays=rays, want=want)


@pytest.fixture(scope="module")
def room(built):
    return make_room()  # traced once, never changed


def observe(room, kind, **opts):
    """One context with `opts` on scene `kind`: every cast in both modes, each held to the oracle.  Returns {(cast, mode): name}."""
    c = capi.Context(0, **opts)
    try:
        if kind == "room_tl":
            c.upload_two_level_scene(room["local"], room["inst"])
        else:
            tris = capi.make_triangles(room["verts"], layers=room["layers"])
            nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(room["verts"]))
            c.upload_scene(tris, nodes, prim_idx)
        cam = capi.camera_look(ORIGIN, FWD, W, H, FOV)
        rays, want, seen = room["rays"], room["want"][kind], {}
        for cast in CASTS:
            flags = capi.FLAG_COHERENT if cast == "coherent" else 0
            got = c.cast_grid(cam, W, H) if cast == "grid" else c.cast(rays, flags=flags)
            seen[(cast, "nearest")] = c.last_kernel_variant()
            parity.assert_exact(got, want, f"{kind} {opts} {cast}: {seen[(cast, 'nearest')]}")
            any_flags = flags | capi.FLAG_BOOL_OUT
            lit = (c.cast_grid(cam, W, H, mode=capi.MODE_ANY_HIT, flags=any_flags) if cast == "grid"
                   else c.cast(rays, mode=capi.MODE_ANY_HIT, flags=any_flags))
            seen[(cast, "any")] = c.last_kernel_variant()
            assert np.array_equal(lit.astype(bool), want["prim_id"] >= 0), f"{kind} {opts} {cast} any-hit: {seen[(cast, 'any')]}"
        return seen
    finally:
        c.close()


def check(seen, names, what):
    for cast, name in zip(CASTS, names):
        for mode, a in (("nearest", "false"), ("any", "true")):
            assert seen[(cast, mode)] == name.replace("{A}", a), (what, cast, mode, seen[(cast, mode)])


@pytest.mark.parametrize("kind", ["room", "room_tl"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_forced_kernel_runs_the_named_instantiation(room, kind, kernel):
    for count_visits in (0, 1):
        seen = observe(room, kind, kernel=KERNELS[kernel], count_visits=bool(count_visits))
        check(seen, EXPECT[(kind, kernel, count_visits)], (kind, kernel, count_visits))


@pytest.mark.parametrize("packet_wg", [64, 256])
@pytest.mark.parametrize("packet_cull", [1, 2])
def test_rows_walk_workgroup_and_culling(room, packet_wg, packet_cull):
    seen = observe(room, "room", kernel=capi.KERNEL_PACKET_DUAL, packet_wg=packet_wg, packet_cull=packet_cull)
    check(seen, EXPECT_DUAL[(packet_wg, packet_cull)], (packet_wg, packet_cull))
