"""mrt_refit_scene / mrt_refit_instanced_scene: new triangles for the resident tree of a flat scene.  A refit tree is a valid BVH over
the new triangles, and results do not depend on which valid BVH is walked (exact ties go to the lower id), so every cast after a
refit must give, bit for bit, what the oracle gives on a fresh build of the new triangles -- ids and layers included, since the
whole row is rewritten.  Every source of a flat scene (host upload, device radix tree, PLOC, SAH), every kernel, an animated room
with shadows, extreme motion, instanced scenes, repeated refits, stream order and the refusals."""
import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po
import parity
import test_shadow_gpu as sh

pytestmark = pytest.mark.gpu
QUAD = pytest.param(capi.KERNEL_PACKET_QUAD, marks=pytest.mark.skipif(not capi.kernel_available(capi.KERNEL_PACKET_QUAD), reason="built without MRT_WITH_QUAD"))
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
SOURCES = {"host": None, "radix_tree": {}, "ploc": {"ploc": True}, "sah": {"sah": True}}
CAM = ((0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0)


def _load(c, v, tris, source):
    """the scene of `tris` (made from v) on c, built by `source`"""
    if SOURCES[source] is None:
        nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(v))
        c.upload_scene(tris, nodes, prim_idx)
    else:
        c.build_scene_device(tris, **SOURCES[source])


def _frame(v, amplitude, phase, seed=3):
    """a displaced copy of v with new ids (reversed) and layers (rotated): a refit rewrites the whole row"""
    n = v.shape[0]
    v1 = synth.deform(v, amplitude, phase, seed)
    ids = (n - 1 - np.arange(n)).astype(np.uint32)
    layers = (1 << ((np.arange(n) + 1) % 3)).astype(np.uint32)
    return v1, ids, layers


def _check(c, osc, name, masks=(0xFFFFFFFF,), brute=False, cam=CAM, wh=(100, 70), incoherent=5000):
    (origin, fwd, fov), (w, h) = cam, wh
    grid = po.grid_rays(origin, fwd, w, h, fov)
    batches = [(grid, "grid")]
    if incoherent:
        inc = synth.incoherent_rays(incoherent, 11)
        inc["origin"] += np.asarray(origin, np.float32) - np.asarray(CAM[0], np.float32)
        batches.append((inc, "incoherent"))
    for rays, kind in batches:
        for mask in masks:
            want = osc.trace(rays, query_mask=mask)
            if brute:
                parity.assert_exact(osc.brute(rays, query_mask=mask), want, f"{name} {kind}: oracle tree vs brute force")
            for flags in (capi.FLAG_COHERENT, 0):
                parity.assert_exact(c.cast(rays, query_mask=mask, flags=flags), want, f"{name} {kind} mask={mask:#x} flags={flags}")
            b = c.cast(rays, query_mask=mask, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
            assert np.array_equal(b.astype(bool), want["prim_id"] >= 0), f"{name} {kind} any-hit"
    camera = capi.camera_look(origin, fwd, w, h, fov)
    want = osc.trace(grid)
    parity.assert_exact(c.cast_grid(camera, w, h), want, f"{name} cast_grid")
    return want


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("n_tris,scale,seed", [(1, 2.0, 5), (2, 2.0, 6), (3, 1.5, 7), (17, 1.0, 8), (1000, 0.5, 1), (20000, 0.25, 33)])
def test_refit_gives_the_oracles_hits_of_the_new_triangles(built, n_tris, scale, seed, source):
    v = synth.soup(n_tris, scale, seed)
    layers = (1 << (np.arange(n_tris) % 3)).astype(np.uint32)
    c = capi.Context(0)
    try:
        _load(c, v, capi.make_triangles(v, None, layers), source)
        v1, ids1, layers1 = _frame(v, 0.3 * scale, 0.9, seed)
        c.refit_scene(capi.make_triangles(v1, ids1, layers1))
        assert c.is_available() and c.scene_info()["n_tris"] == n_tris
        assert c.stats()["last_build_ms"] > 0.0
        want = _check(c, po.OracleScene(v1, ids1, layers1), f"{source} n={n_tris}", masks=(0xFFFFFFFF, 0x5), brute=n_tris <= 17)
        assert (want["prim_id"] >= 0).any()
    finally:
        c.close()


@pytest.mark.parametrize("kernel", [capi.KERNEL_LANE, capi.KERNEL_PACKET, capi.KERNEL_PACKET_ASM, capi.KERNEL_PACKET_DUAL, capi.KERNEL_PACKET_ROWS,
                                    QUAD, capi.KERNEL_LANE_PERSISTENT, capi.KERNEL_LANE4_PERSISTENT, capi.KERNEL_LANE8_PERSISTENT])
def test_every_kernel_walks_a_refit_host_tree(built, kernel):
    """A host-uploaded scene's compact 4- and 8-wide layouts are re-derived at binary-node indices by its first refit, and its row
    arrays rebuilt: every walk must still give the oracle's hits, after the first refit and after a second one in place."""
    v = synth.soup(3000, 0.35, 17)
    c = capi.Context(0, kernel=kernel)
    try:
        _load(c, v, capi.make_triangles(v), "host")
        for phase in (0.4, 2.1):
            v1, ids1, layers1 = _frame(v, 0.1, phase)
            c.refit_scene(capi.make_triangles(v1, ids1, layers1))
            _check(c, po.OracleScene(v1, ids1, layers1), f"kernel={kernel} phase={phase}", masks=(0xFFFFFFFF, 0x3))
    finally:
        c.close()


def _room_frame(local, inst, f):
    """frame f of the room: the sphere rolls along a circle, the turned box slides and turns, the pillar bobs"""
    a = 0.45 * f
    moved = inst.copy()
    moved[6]["origin"] = inst[6]["origin"] + np.array([0.8 * np.sin(a), 0.0, 0.8 * np.cos(a) - 0.8], np.float32)
    ca, sa = np.float32(np.cos(0.3 * a)), np.float32(np.sin(0.3 * a))
    turn = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]], np.float32)
    moved[7]["basis"] = (turn @ inst[7]["basis"].reshape(3, 3)).astype(np.float32).reshape(9)
    moved[7]["origin"] = inst[7]["origin"] + np.array([0.3 * f, 0.0, -0.2 * f], np.float32)
    moved[8]["origin"] = inst[8]["origin"] + np.array([0.0, 0.25 * np.sin(a), 0.0], np.float32)
    return synth.flatten_instances(local, moved)


def test_animated_room_with_shadows(built):
    """Eight frames of synth.room() with the sphere and the boxes moving, refit frame after frame from the host-built tree of frame 0:
    the primary grid and the shadow masks of two lights against the oracle every frame."""
    local, inst = synth.room()
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    (origin, fwd, fov), (w, h) = sh.ROOM_CAM, (160, 120)
    cam = capi.camera_look(origin, fwd, w, h, fov)
    rays = po.grid_rays(origin, fwd, w, h, fov)
    lights = np.concatenate([sh.light(T.LIGHT_DIRECTIONAL, direction=(0.3, 1.0, 0.2)), sh.light(T.LIGHT_POINT, pos=(1.0, 4.5, 1.5))])
    c = capi.Context(0)
    d_hits, d_mask = c.device_alloc(w * h * 32), c.device_alloc(w * h * len(lights))
    try:
        v0 = _room_frame(local, inst, 0)
        _load(c, v0, capi.make_triangles(v0, None, layers), "host")
        for f in range(8):
            v = _room_frame(local, inst, f)
            if f:
                c.refit_scene(capi.make_triangles(v, None, layers))
            osc = po.OracleScene(v, None, layers)
            want = osc.trace(rays)
            c.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
            got = np.zeros(w * h, dtype=T.HIT32)
            c.d2h(got, d_hits)
            parity.assert_exact(got, want, f"room frame {f}")
            hit = want["prim_id"] >= 0
            with np.errstate(over="ignore", invalid="ignore"):  # (the position of a miss is not used)
                pos = rays["origin"] + rays["direction"] * want["t"][:, None]
            srays, traced = sh.shadow_rays(pos, want["normal"], hit, lights)
            lit = (~(traced & (osc.trace(srays, any_hit=True)["prim_id"] >= 0))).astype(np.uint8)
            assert lit.min() == 0 and lit.max() == 1
            c.cast_grid_shadows(cam, w, h, d_hits, lights, d_mask)
            mask = np.zeros(w * h * len(lights), dtype=np.uint8)
            c.d2h(mask, d_mask)
            np.testing.assert_array_equal(mask, lit, err_msg=f"room frame {f} shadows")
    finally:
        c.device_free(d_hits); c.device_free(d_mask)
        c.close()


@pytest.mark.parametrize("kernel", [capi.KERNEL_AUTO, capi.KERNEL_PACKET_DUAL])
def test_scene_moved_far_away(built, kernel):
    """The whole scene translated 1e3 units (and the camera with it): the packet walk's frustum cull takes its error bound from the
    scene's bounds, which the refit must carry, or a hit near the new coordinates could be culled."""
    v = synth.soup(20000, 0.25, 41)
    c = capi.Context(0, kernel=kernel)
    try:
        _load(c, v, capi.make_triangles(v), "host")
        far = (v + np.float32(1000.0)).astype(np.float32)
        c.refit_scene(capi.make_triangles(far))
        cam = (tuple(np.asarray(CAM[0], np.float32) + np.float32(1000.0)), CAM[1], CAM[2])
        want = _check(c, po.OracleScene(far), f"far kernel={kernel}", cam=cam, wh=(256, 192))
        assert (want["prim_id"] >= 0).sum() > 1000
    finally:
        c.close()


@pytest.mark.parametrize("source", ["host", "radix_tree", "sah"])
def test_shuffled_and_collapsed_triangles(built, source):
    """Vertices shuffled among the triangles (every leaf box now spans the scene: a terrible, still valid tree), then triangles
    collapsed to points (half of them, then all: boxes of one point, no hits from them)."""
    v = synth.soup(5000, 0.3, 12)
    c = capi.Context(0)
    try:
        _load(c, v, capi.make_triangles(v), source)
        perm = np.random.default_rng(5).permutation(v.shape[0])
        shuffled = v[perm]
        c.refit_scene(capi.make_triangles(shuffled))
        _check(c, po.OracleScene(shuffled), f"{source} shuffled", incoherent=2000)
        points = v.copy()
        points[::2] = v[::2].mean(axis=1, keepdims=True)
        c.refit_scene(capi.make_triangles(points))
        _check(c, po.OracleScene(points), f"{source} half points", incoherent=2000)
        points[:] = v.mean(axis=1, keepdims=True)
        c.refit_scene(capi.make_triangles(points))
        want = _check(c, po.OracleScene(points), f"{source} all points", incoherent=2000)
        assert not (want["prim_id"] >= 0).any()
    finally:
        c.close()


def test_refit_instanced_scene(built):
    """build_instanced_scene_device, then refit_instanced_scene with deformed meshes and new transforms (meshes on the host, then
    resident on the device): the oracle of the flattened new instances."""
    local, inst = synth.multi_mesh_instances(8, 2000, 0.1, 7)
    extra = inst[[0, 3]].copy()                       # meshes 0 and 3 placed a second time
    extra["origin"] += np.array([0.5, -0.25, 1.0], dtype=np.float32)
    extra["layers"] = [0x2, 0x4]
    inst = np.concatenate([inst, extra])
    c = capi.Context(0)
    d_local = None
    try:
        c.build_instanced_scene_device(local, inst)
        for step, on_device in ((1, False), (2, True)):
            moved = inst.copy()
            moved["origin"] += np.float32(0.2 * step) * synth.uniform01(50 + step, 0, 3 * len(inst)).reshape(-1, 3) - np.float32(0.1 * step)
            ang = np.float32(0.2 * step)
            rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], np.float32)
            moved["basis"][1] = (rz @ inst["basis"][1].reshape(3, 3)).astype(np.float32).reshape(9)
            moved["layers"][2] = 0x6
            new_local = synth.deform(local, 0.05, 0.6 * step, seed=step)
            world = synth.flatten_instances(new_local, moved)
            n = world.shape[0]
            ids = np.arange(n, dtype=np.uint32)
            layers = np.repeat(moved["layers"], moved["n_tris"]).astype(np.uint32)
            assert po.flatten_instances(new_local, moved).tobytes() == capi.make_triangles(world, ids, layers).tobytes()
            if on_device:
                d_local = c.device_alloc(new_local.nbytes)
                c.h2d(d_local, new_local)
                c.refit_instanced_scene(d_local, moved, n_mesh_tris=new_local.shape[0], on_device=True)
            else:
                c.refit_instanced_scene(new_local, moved)
            _check(c, po.OracleScene(world, ids, layers), f"instanced step {step}", masks=(0xFFFFFFFF, 0x2))
        with pytest.raises(capi.MrtError) as e:                 # one instance fewer: not the scene's triangle count
            c.refit_instanced_scene(local, inst[:-1])
        assert e.value.status == capi.ERR_INVALID
    finally:
        if d_local is not None:
            c.device_free(d_local)
        c.close()


def _records(c, grid, inc):
    cam = capi.camera_look(CAM[0], CAM[1], 100, 70, CAM[2])
    return [c.cast(grid, flags=capi.FLAG_COHERENT).tobytes(), c.cast(inc).tobytes(), c.cast_grid(cam, 100, 70).tobytes(),
            c.cast(inc, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT).tobytes()]


@pytest.mark.parametrize("source", ["host", "radix_tree"])
def test_identity_refit_and_no_drift(built, source, monkeypatch):
    """A refit with the scene's own triangles changes no byte of any record; ten refits in a row between two frames come back to
    the same records every time (every cast's output first filled with a pattern no kernel writes: MRT_POISON_OUTPUT)."""
    v = synth.soup(20000, 0.25, 9)
    tris = capi.make_triangles(v)
    grid, inc = po.grid_rays(CAM[0], CAM[1], 100, 70, CAM[2]), synth.incoherent_rays(5000, 11)
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")
    c = capi.Context(0)
    try:
        _load(c, v, tris, source)
        before = _records(c, grid, inc)
        c.refit_scene(tris)
        assert _records(c, grid, inc) == before
        v1, ids1, layers1 = _frame(v, 0.1, 1.3)
        other = capi.make_triangles(v1, ids1, layers1)
        c.refit_scene(other)
        _check(c, po.OracleScene(v1, ids1, layers1), f"{source} frame B")
        after = _records(c, grid, inc)
        for k in range(10):
            c.refit_scene(tris if k % 2 == 0 else other)
            assert _records(c, grid, inc) == (before if k % 2 == 0 else after), f"refit {k}"
    finally:
        c.close()


def test_stream_order_and_refusals(built):
    v = synth.soup(4000, 0.3, 21)
    tris = capi.make_triangles(v)
    v1, ids1, layers1 = _frame(v, 0.2, 0.5)
    new = capi.make_triangles(v1, ids1, layers1)
    old_osc, new_osc = po.OracleScene(v), po.OracleScene(v1, ids1, layers1)
    grid = po.grid_rays(CAM[0], CAM[1], 100, 70, CAM[2])
    n = grid.shape[0]
    c = capi.Context(0)
    ptrs = []
    try:
        with pytest.raises(capi.MrtError) as e:                         # no scene
            c.refit_scene(tris)
        assert e.value.status == capi.ERR_NO_SCENE
        _load(c, v, tris, "host")
        # a cast queued with MRT_FLAG_ASYNC before the refit sees the old triangles, a cast after it the new ones
        d_rays, d_a, d_b = c.device_alloc(grid.nbytes), c.device_alloc(n * 32), c.device_alloc(n * 32)
        ptrs += [d_rays, d_a, d_b]
        c.h2d(d_rays, grid)
        c.cast(d_rays, d_a, count=n, flags=DEV | capi.FLAG_COHERENT | capi.FLAG_ASYNC)
        c.refit_scene(new)
        c.cast(d_rays, d_b, count=n, flags=DEV | capi.FLAG_COHERENT)
        a, b = np.zeros(n, dtype=T.HIT32), np.zeros(n, dtype=T.HIT32)
        c.d2h(a, d_a); c.d2h(b, d_b)
        parity.assert_exact(a, old_osc.trace(grid), "async cast queued before the refit")
        parity.assert_exact(b, new_osc.trace(grid), "cast after the refit")
        assert c.stats()["last_build_ms"] > 0.0
        c.refit_scene(tris)
        # a pending submit: refused until it is collected
        c.submit(grid)
        with pytest.raises(capi.MrtError) as e:
            c.refit_scene(new)
        assert e.value.status == capi.ERR_PENDING
        parity.assert_exact(c.collect(), old_osc.trace(grid), "collected after the refused refit")
        # refusals leave the scene as it was
        bad_nan, bad_inf = tris.copy(), tris.copy()
        bad_nan["v0"][123, 1] = np.nan
        bad_inf["edge2"][7, 0] = np.inf
        for bad, status in ((tris[:-1], capi.ERR_INVALID), (bad_nan, capi.ERR_INVALID), (bad_inf, capi.ERR_INVALID)):
            with pytest.raises(capi.MrtError) as e:
                c.refit_scene(bad)
            assert e.value.status == status
            _check(c, old_osc, "after a refused refit", incoherent=1000)
        assert "non-finite" in str(e.value)
        assert c.L.mrt_refit_scene(c.h, capi._np(tris), tris.shape[0], capi.BUILD_SAH) == capi.ERR_INVALID  # no such flag here
        _check(c, old_osc, "after a refused flag", incoherent=1000)
        # a two-level scene is refused
        local, inst = synth.multi_mesh_instances(4, 500, 0.3, 5)
        c.upload_two_level_scene(local, inst)
        world = capi.make_triangles(synth.flatten_instances(local, inst))
        for call in (lambda: c.refit_scene(world), lambda: c.refit_instanced_scene(local, inst)):
            with pytest.raises(capi.MrtError) as e:
                call()
            assert e.value.status == capi.ERR_UNSUPPORTED
        want = po.OracleTwoLevelScene(local, inst).trace(grid)
        parity.assert_exact(c.cast(grid, flags=capi.FLAG_COHERENT), want, "two-level scene after the refused refit")
    finally:
        for p in ptrs:
            c.device_free(p)
        c.close()
