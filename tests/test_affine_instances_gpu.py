"""Every device form of the two-level walk, every way a two-level scene is made and every record-driven cast, on mirrored,
non-uniformly scaled and sheared instances (tests/affine_scene.py).  The oracle's two-level walk is the specification -- pinned to a
float64 brute force on this very scene by tests/test_affine_instances_cpu.py -- and the device is held to it bit for bit
(parity.assert_exact): the mesh-space ray of the lane, packet (shared-octant walker and mixed-octant fallback) and resident-wave
forms, the token expansion's second Moller-Trumbore, normalize(basis . n_mesh), the top level built on the host and in the three
device forms, the refit, and the four source kernels that make rays from such records.

Ray counts are small (grids 96x72 and a clipped 61x37, 4 000 incoherent rays) but for one batch of 2^16 rays: the smallest an
MRT_KERNEL_AUTO context walks with resident waves (launch_policy.cpp plan_cast: `auto_k && n >= 65536`).

Measured on an MI355X: no record of any cast in this file differs from the oracle's in any bit, and the expanded tokens are the walks'
own records.  The flat walk's normal (the flattened triangle's own) against the two-level record's normal of the same triangle, device
records of both contexts, 96x72 grid: rigid 0.9999999 .. 1, mirror -1 .. -0.9999999, nonuniform 0.464 .. 0.9979, shear 0.663 .. 0.9984,
mirror_nonuni -0.9977 .. -0.461 (the oracle's figures: tests/test_affine_instances_cpu.py)."""
import numpy as np
import pytest

import affine_scene as A
import layout_check as lc
import parity
import test_bounce_gpu as bn
import test_hemisphere_gpu as hm
import test_reflections_gpu as rf
import test_shadow_gpu as sh
from messyerraytracer_amd import capi, synth, types as T
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

RESIDENT_MIN_RAYS = 1 << 16          # launch_policy.cpp: a sorted batch takes the persistent lane kernels from here on
PACKET, LANE, RESIDENT = "trace_two_level_packet_kernel<", "trace_two_level_kernel<", "trace_lane_persistent_kernel<"


class Shared:
    """the scene, its ray sets and what the oracle says of them, per set of instances; computed once, never changed"""

    def __init__(self):
        self.sc = A.scene()
        # before any cast: the packet walk's octant choice has both kinds of work on this scene -- instances whose mesh-space directions
        # M d share one sign pattern across a tile (the shared-octant walker) and instances for which they are mixed within a tile (the
        # fallback); whole 8x8 tiles, and the 2x2-pixel pieces an MRT_KERNEL_AUTO context casts a grid this small in
        for tile in (8, 2):
            uniform, mixed = self.sc.tile_octants(*A.GRID, tile=tile)
            assert uniform > 0 and mixed > 0, (tile, uniform, mixed)
        self.rays = {"grid": self.sc.grid_rays(*A.GRID), "clipped": self.sc.grid_rays(*A.CLIPPED),
                     "incoherent": self.sc.incoherent_rays(4000), "big": synth.incoherent_rays(RESIDENT_MIN_RAYS, 13)}
        self.cams = {"grid": capi.camera_look(A.CAM[0], A.CAM[1], *A.GRID, A.CAM[2]),
                     "clipped": capi.camera_look(A.CAM[0], A.CAM[1], *A.CLIPPED, A.CAM[2])}
        self.rigid = self.sc.rigid_instances()
        self.deformed = synth.deform(self.sc.local, 0.05, 1.0, seed=4)
        self._oracles, self._want = {}, {}

    def oracle(self, which):
        if which not in self._oracles:
            local, inst = {"affine": (self.sc.local, self.sc.inst), "rigid": (self.sc.local, self.rigid),
                           "deformed": (self.deformed, self.sc.inst)}[which]
            self._oracles[which] = po.OracleTwoLevelScene(local, inst)
        return self._oracles[which]

    def want(self, name, mask=0xFFFFFFFF, which="affine"):
        key = (which, name, mask)
        if key not in self._want:
            self._want[key] = self.oracle(which).trace(self.rays[name], query_mask=mask)
            assert int((self._want[key]["prim_id"] >= 0).sum()) > 100, key
        return self._want[key]


@pytest.fixture(scope="module")
def S(built):
    return Shared()


class Bufs:
    def __init__(self, c):
        self.c, self.ptrs = c, []

    def alloc(self, nbytes):
        p = self.c.device_alloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def put(self, arr):
        p = self.alloc(arr.nbytes)
        self.c.h2d(p, np.ascontiguousarray(arr))
        return p

    def get(self, p, n, dtype):
        out = np.zeros(n, dtype=dtype)
        self.c.d2h(out, p)
        return out

    def free(self):
        for p in self.ptrs:
            self.c.device_free(p)
        self.ptrs = []


# ---- every walk, named -------------------------------------------------------------------------------------------------------------

# (kernel, stack_override) -> the instantiations that must have run in that context (prefix, and what the name must contain)
WALKS = {
    "auto": (capi.KERNEL_AUTO, 0, {"grid": (PACKET, ""), "plain": (LANE, ""), "big": (RESIDENT, ", 8, true")}),
    "lane": (capi.KERNEL_LANE, 0, {"grid": (LANE, ""), "plain": (LANE, ""), "big": (LANE, "")}),
    "lane8_persistent": (capi.KERNEL_LANE8_PERSISTENT, 0, {"grid": (PACKET, ""), "plain": (RESIDENT, ", 8, true"), "big": (RESIDENT, ", 8, true")}),
    "auto_stack4": (capi.KERNEL_AUTO, 4, {"grid": (PACKET, ""), "plain": (LANE, ""), "big": (RESIDENT, ", 8, true")}),
}


@pytest.mark.parametrize("walk", list(WALKS))
def test_every_walk_gives_the_oracles_records(S, walk):
    """mrt_cast_grid, mrt_cast(COHERENT) and plain mrt_cast under each kernel option, three query masks, any-hit bytes; the named
    instantiations observed through last_kernel_variant(): the packet kernel (whole tiles under a forced kernel, pieces under AUTO),
    the lane kernel, the 8-wide persistent form (which starts from the instance's other root) and the resident form of the 2^16 batch
    (with 4 stack entries in LDS: the rest spills to HBM)."""
    kernel, stack, named = WALKS[walk]
    c = capi.Context(0, kernel=kernel, stack_override=stack)
    seen = {}
    try:
        c.upload_two_level_scene(S.sc.local, S.sc.inst)
        for mask in A.MASKS:
            for name in ("grid", "clipped"):
                want, (w, h) = S.want(name, mask), (A.GRID if name == "grid" else A.CLIPPED)
                parity.assert_exact(c.cast_grid(S.cams[name], w, h, query_mask=mask), want, f"{walk} cast_grid {name} mask={mask:#x}")
                seen.setdefault("grid", c.last_kernel_variant())
                b = c.cast_grid(S.cams[name], w, h, query_mask=mask, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
                assert np.array_equal(b.astype(bool), want["prim_id"] >= 0), f"{walk} cast_grid any-hit {name} mask={mask:#x}"
            for name in ("grid", "clipped", "incoherent"):
                want, rays = S.want(name, mask), S.rays[name]
                parity.assert_exact(c.cast(rays, query_mask=mask, flags=capi.FLAG_COHERENT), want, f"{walk} coherent {name} mask={mask:#x}")
                parity.assert_exact(c.cast(rays, query_mask=mask), want, f"{walk} plain {name} mask={mask:#x}")
                seen.setdefault("plain", c.last_kernel_variant())
                for flags in (capi.FLAG_COHERENT, 0):
                    b = c.cast(rays, query_mask=mask, mode=capi.MODE_ANY_HIT, flags=flags | capi.FLAG_BOOL_OUT)
                    assert np.array_equal(b.astype(bool), want["prim_id"] >= 0), f"{walk} any-hit {name} mask={mask:#x} flags={flags}"
        want = S.want("big")
        parity.assert_exact(c.cast(S.rays["big"]), want, f"{walk} 2^16 rays")
        seen["big"] = c.last_kernel_variant()
        b = c.cast(S.rays["big"], mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        assert np.array_equal(b.astype(bool), want["prim_id"] >= 0), f"{walk} 2^16 rays any-hit"
        for cast, (prefix, part) in named.items():
            assert seen[cast].startswith(prefix) and part in seen[cast], (walk, cast, seen[cast])
    finally:
        c.close()


@pytest.mark.parametrize("kernel", [capi.KERNEL_AUTO, capi.KERNEL_LANE8_PERSISTENT], ids=["auto", "lane8_persistent"])
def test_host_layout_records_and_tokens(S, kernel):
    """44-byte records from 60-byte rays against po.unpack_hits; MRT_FLAG_TOKEN_OUT followed by mrt_expand_tokens: the expansion
    redoes Moller-Trumbore in mesh space and must rebuild the walk's own records byte for byte."""
    c = capi.Context(0, kernel=kernel)
    d = Bufs(c)
    try:
        c.upload_two_level_scene(S.sc.local, S.sc.inst)
        assert c.token_bytes() == 8
        for name in ("grid", "incoherent", "big"):
            rays, want = S.rays[name], S.want(name)
            n = rays.shape[0]
            if name != "big":
                host = po.make_host_rays(rays)
                assert c.cast(host, flags=capi.FLAG_HOST_LAYOUT).tobytes() == po.unpack_hits(want, host).tobytes(), f"{name} host layout"
            d_rays, d_tok, d_hits = d.put(rays), d.alloc(n * 8), d.alloc(n * 32)
            for flags in (capi.FLAG_COHERENT, 0):
                own = c.cast(rays, flags=flags)
                tok = c.cast(rays, flags=flags | capi.FLAG_TOKEN_OUT)
                assert tok.shape == (n, 2) and np.array_equal(tok[:, 0] != capi.TOKEN_MISS, want["prim_id"] >= 0)
                c.h2d(d_tok, tok)
                c.expand_tokens(d_rays, d_tok, d_hits, n)
                c.synchronize()
                got = d.get(d_hits, n, T.HIT32)
                assert got.tobytes() == own.tobytes(), f"{name} flags={flags}: expanded tokens are not the walk's own records"
                parity.assert_exact(got, want, f"{name} flags={flags} expanded tokens")
            d.free()
        # the grid form: tokens written by mrt_cast_grid, records rebuilt from the camera
        (w, h), want = A.GRID, S.want("grid")
        d_tok, d_hits = d.alloc(w * h * 8), d.alloc(w * h * 32)
        c.cast_grid(S.cams["grid"], w, h, hits=d_tok, flags=capi.FLAG_HITS_ON_DEVICE | capi.FLAG_TOKEN_OUT)
        c.expand_grid_tokens(S.cams["grid"], w, h, 0, h, d_tok, d_hits)
        c.synchronize()
        assert d.get(d_hits, w * h, T.HIT32).tobytes() == want.tobytes()
    finally:
        d.free()
        c.close()


# ---- every way the scene is made -----------------------------------------------------------------------------------------------------

def made(c, S, local, inst, leaf_boxes, which, what):
    """the snapshot through the validator, then the grid and the incoherent rays against the oracle of (local, inst)"""
    findings = lc.check_two_level(c.debug_snapshot(), local, inst, leaf_boxes=leaf_boxes)
    assert not findings, f"{what}:\n{lc.summary(findings)}"
    parity.assert_exact(c.cast_grid(S.cams["grid"], *A.GRID), S.want("grid", which=which), f"{what} cast_grid")
    parity.assert_exact(c.cast(S.rays["grid"], flags=capi.FLAG_COHERENT), S.want("grid", which=which), f"{what} coherent grid")
    parity.assert_exact(c.cast(S.rays["incoherent"]), S.want("incoherent", which=which), f"{what} incoherent")


UPLOADS = {"host": ({}, "host"), "radix": ({"blas_on_device": True}, "device"), "sah": ({"blas_on_device": True, "sah": True}, "device")}


@pytest.mark.parametrize("upload", list(UPLOADS))
def test_uploads(S, upload):
    kw, boxes = UPLOADS[upload]
    c = capi.Context(0)
    try:
        c.upload_two_level_scene(S.sc.local, S.sc.inst, **kw)
        made(c, S, S.sc.local, S.sc.inst, boxes, "affine", f"{upload} upload")
        parity.assert_exact(c.cast(S.rays["big"]), S.want("big"), f"{upload} upload 2^16 rays")   # the 8-wide BLAS layout of this upload
        assert c.last_kernel_variant().startswith(RESIDENT), c.last_kernel_variant()
    finally:
        c.close()


def test_update_instances_from_rigid_to_affine_and_back(S):
    c = capi.Context(0)
    try:
        c.upload_two_level_scene(S.sc.local, S.rigid)
        made(c, S, S.sc.local, S.rigid, "host", "rigid", "rigid upload")
        for step in range(2):
            c.update_instances(S.sc.inst)
            made(c, S, S.sc.local, S.sc.inst, "host", "affine", f"update to affine {step}")
            c.update_instances(S.rigid)
            made(c, S, S.sc.local, S.rigid, "host", "rigid", f"update back to rigid {step}")
    finally:
        c.close()


@pytest.mark.parametrize("form", list(capi.TLAS_FORMS))
def test_update_instances_device(S, form):
    """the top level built on the device in each form, from a host array and from a device pointer"""
    c = capi.Context(0)
    d = Bufs(c)
    try:
        c.upload_two_level_scene(S.sc.local, S.rigid)
        d_inst = d.put(S.sc.inst)
        for on_device in (False, True):
            c.update_instances(S.rigid)
            if on_device:
                c.update_instances_device(d_inst, on_device=True, form=form, n_instances=S.sc.inst.shape[0])
            else:
                c.update_instances_device(S.sc.inst, form=form)
            made(c, S, S.sc.local, S.sc.inst, "host", "affine", f"{form} on_device={on_device}")
        parity.assert_exact(c.cast(S.rays["big"]), S.want("big"), f"{form} 2^16 rays")
        c.update_instances_device(S.rigid, form=form)
        made(c, S, S.sc.local, S.rigid, "host", "rigid", f"{form} back to rigid")
    finally:
        d.free()
        c.close()


@pytest.mark.parametrize("instances_on_device", [False, True], ids=["host_instances", "device_instances"])
def test_refit_with_deformed_meshes(S, instances_on_device):
    """mrt_refit_two_level_scene: every mesh's vertices move (synth.deform), the instances are the affine ones; from a rigid upload, so
    that the refit's top level is the first to see them"""
    c = capi.Context(0)
    d = Bufs(c)
    try:
        c.upload_two_level_scene(S.sc.local, S.rigid)
        if instances_on_device:
            c.refit_two_level_scene(S.deformed, d.put(S.sc.inst), instances_on_device=True, n_instances=S.sc.inst.shape[0])
        else:
            c.refit_two_level_scene(S.deformed, S.sc.inst)
        made(c, S, S.deformed, S.sc.inst, "device", "deformed", f"refit instances_on_device={instances_on_device}")
        parity.assert_exact(c.cast(S.rays["big"]), S.want("big", which="deformed"), "refit 2^16 rays")   # the re-derived 8-wide layout
        c.refit_two_level_scene(S.sc.local, S.sc.inst)
        made(c, S, S.sc.local, S.sc.inst, "device", "affine", "refit back to the first vertices")
    finally:
        d.free()
        c.close()


# ---- the flat side -------------------------------------------------------------------------------------------------------------------

def test_flattened_scene_and_the_other_normal_convention(S):
    """mrt_flatten_instances equals synth.flatten_instances bit for bit; the flat scene built from it casts po.OracleScene's records,
    whose normal is the world triangle's own: against the two-level context's records, the relation of every class."""
    sc = S.sc
    n = sc.world.shape[0]
    flat, two = capi.Context(0), capi.Context(0)
    d = Bufs(flat)
    try:
        d_out = d.alloc(n * 64)
        flat.flatten_instances(sc.local, sc.inst, d_out)
        got = d.get(d_out, n, T.TRI64)
        assert np.array_equal(got["v0"].view(np.uint32), sc.world[:, 0].view(np.uint32))
        assert got.tobytes() == capi.make_triangles(sc.world, sc.ids, sc.layers).tobytes() == sc.tris.tobytes()
        flat.build_instanced_scene_device(sc.local, sc.inst)
        osc = po.OracleScene(sc.world, sc.ids, sc.layers)
        records = {}
        for mask in A.MASKS:
            for name in ("grid", "clipped"):
                w, h = A.GRID if name == "grid" else A.CLIPPED
                records[name, mask] = flat.cast_grid(S.cams[name], w, h, query_mask=mask)
                parity.assert_exact(records[name, mask], osc.trace(S.rays[name], query_mask=mask), f"flat cast_grid {name} mask={mask:#x}")
            for flags in (capi.FLAG_COHERENT, 0):
                parity.assert_exact(flat.cast(S.rays["incoherent"], query_mask=mask, flags=flags), osc.trace(S.rays["incoherent"], query_mask=mask),
                                    f"flat incoherent mask={mask:#x} flags={flags}")
        parity.assert_exact(flat.cast(S.rays["big"]), osc.trace(S.rays["big"]), "flat 2^16 rays")
        two.upload_two_level_scene(sc.local, sc.inst)
        tl = two.cast_grid(S.cams["grid"], *A.GRID)
        for name, (lo, hi) in A.normal_relation(sc, tl, records["grid", 0xFFFFFFFF]).items():
            print(f"{name}: dot {lo:.7g} .. {hi:.7g}")
    finally:
        d.free()
        flat.close(); two.close()


# ---- record-driven casts -------------------------------------------------------------------------------------------------------------

def test_shadows_from_affine_records(built):
    w, h = A.GRID
    sh.check_entry_points("affine_tl", w, h, 0, h, variant=sh.PLAIN["affine_tl"])


def test_reflections_from_affine_records(built):
    rf.check_all_entry_points("affine_tl", *A.GRID, variant=rf.PLAIN["affine_tl"])


def test_hemisphere_from_affine_records(built):
    hm.check_all_entry_points("affine_tl", *A.GRID, variant=hm.PLAIN["affine_tl"])


def test_bounce_from_affine_records(built):
    bn.check_all_entry_points("affine_tl", *A.GRID, variant=bn.PLAIN["affine_tl"])
