"""Shadow and reflection casts on hand-made records at the edges of their formulas: the 1e-6 threshold from both sides, distances that
overflow, zero, denormal and -0.0 lights and normals, positions at 1e30, n . d == +-0, zero normals, non-unit and huge incoming
directions, misses whose other fields hold garbage, select bytes other than 0 and 1 (tests/source_edge_cases.py; the lights and the
shadow edge records are those of tests/golden/shadow_reference.npz, which test_shadow_cpu.py holds to the reference's own text).
Expected values: messyerraytracer_amd/shadow.py and reflection.py traced by the oracle, byte for byte, in every source layout, in the
plain kernels and in the persistent ones, flat and two-level synth.room() (lowered, so that the origin is in free space).  Every context has MRT_POISON_OUTPUT set, so a byte or a
record no kernel wrote shows."""
import os

import numpy as np
import pytest

from messyerraytracer_amd import capi, synth, types as T
from messyerraytracer_amd import reflection as R
from messyerraytracer_amd import shadow as S
from oracle import pyoracle as po
import source_edge_cases as E
from test_shadow_gpu import Dev, Scene

pytestmark = pytest.mark.gpu

F = np.float32
N, W, H = E.N, 64, 64
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
CAM = ((0.0, 0.0, 0.0), (0.0, -0.3, -1.0), 70.0)  # at the origin: a grid record with t = 0 sits at position 0 exactly
MAX_DIST = F(25.0)
SRC_RAY32, SRC_HOST44, SRC_GRID = 1, 2, 3         # the shadow sources as mrt_last_kernel_variant numbers them
PLAIN = {"room": "trace_shadow_lane_kernel<%d>", "room_tl": "trace_shadow_two_level_kernel<%d>"}
PERSISTENT = "trace_shadow_persistent_kernel<%d, %d, %s>"
CACHE = {}


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")


def cached(key, make):
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def scene(kind):
    """synth.room() flat ("room") or two-level ("room_tl"), lowered by source_edge_cases.LOWER (every instance's origin; the flat scene
    flattened from those instances)"""
    def make():
        sc = Scene(kind)
        sc.inst = sc.inst.copy()
        sc.inst["origin"][:, 1] -= E.LOWER
        sc.verts = synth.flatten_instances(sc.local, sc.inst)
        return sc
    return cached(("scene", kind), make)


def golden():
    def load():
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shadow_reference.npz")) as z:
            return {k: z[k] for k in z.files}
    return cached("golden", load)


def same(a, b, what=""):
    """byte for byte; a failure names the first rows that differ and shows both sides"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize
    rows = a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)
    bad = np.flatnonzero(rows.any(axis=1))
    assert bad.size == 0, "%s: %d of %d rows differ, first %s\ngot  %s\nwant %s" % (what, bad.size, a.shape[0], bad[:8], a[bad[:8]], b[bad[:8]])


def oracle(kind, rays, any_hit=False):
    """The oracle's walk -- where its answer does not hang on a tie that the boxes decide.  A ray that ends on a triangle at t = t_max
    exactly, or whose nearest hit lies on two coplanar faces at once (the turned box rests on the floor), gets the answer of whichever
    subtree is visited first: a later box test against the t found so far can round either way.  Such a ray has no expected value and
    does not belong in these tests, so: on the flat scene the brute-force loop must agree (hit or miss; closest-hit: the whole
    record), on the two-level scene the same walk over the instances in reverse order must find the same hit."""
    sc = scene(kind)
    if sc._oracle is None:
        sc.oracle_any(rays[:1])   # (builds it)
    hits = sc._oracle.trace(rays, any_hit=any_hit)
    if not sc.two_level:
        brute = sc._oracle.brute(rays, any_hit=any_hit)
        if any_hit:
            np.testing.assert_array_equal(hits["prim_id"] >= 0, brute["prim_id"] >= 0)
        else:
            same(hits, brute, "walk and brute force")
    elif not any_hit:
        other = cached("reversed", lambda: po.OracleTwoLevelScene(sc.local, sc.inst[::-1].copy())).trace(rays)
        for f in ("t", "bary_u", "bary_v", "normal", "hit_layers"):   # (the flat ids differ: they count from the instance order)
            same(hits[f], other[f], "instances in reverse order, " + f)
    return hits


def hit_point(rays, t):
    with np.errstate(all="ignore"):
        return rays["origin"] + rays["direction"] * t[:, None]


# ---------------------------------------------------------------------------------------------------------------- shadows

class ShadowInputs:
    """The N records in the three source layouts, and the position each layout's kernel derives for them."""

    def __init__(self):
        self.pos, self.nrm, self.hit = E.shadow_records(golden())
        # mrt_hit32 + rays from an array: o = 0, d = position, t = 1 (the product is exact)
        self.rays = E.rays32(np.zeros((N, 3), dtype=F), self.pos)
        self.rec32 = E.records32(self.nrm, self.hit, np.ones(N, dtype=F))
        # mrt_host_hit44: the position itself (the rays are not read)
        self.hrays = po.make_host_rays(E.rays32(np.zeros((N, 3), dtype=F), np.where(self.hit[:, None], self.pos, F(1))))
        self.rec44 = E.records44(self.pos, self.nrm, self.hit)
        # the grid source: the records of a 64 x 64 camera grid overwritten by hand; positions o + d * t of the camera's rays
        self.grid_rays = po.grid_rays(CAM[0], CAM[1], W, H, CAM[2])
        self.grid_t = E.grid_distances()
        self.grid32 = E.records32(self.nrm, self.hit, self.grid_t)
        self.positions = {SRC_RAY32: hit_point(self.rays, np.ones(N, dtype=F)), SRC_HOST44: self.pos,
                          SRC_GRID: hit_point(self.grid_rays, self.grid_t)}
        self.calls = E.shadow_light_calls(golden())
        # four lights: at the origin, at dist 1e-6 exactly from it, an ordinary one, the one with cast_shadows == 0
        self.four = np.concatenate([self.calls[0][[0, 6]], self.calls[1][[12]], self.calls[0][[15]]])
        assert self.four["cast_shadows"][3] == 0 and self.calls[0]["cast_shadows"][15] == 0
        assert (self.grid_t == 0).any() and not self.hit.all()


def shadow_inputs():
    return cached("shadow_inputs", ShadowInputs)


def shadow_expected(kind, src, lights_key):
    """(mask, traced, rays) of one call: shadow.py on the positions source `src` derives, traced any-hit by the oracle of the scene"""
    def make():
        inp = shadow_inputs()
        lights = inp.four if lights_key == "four" else inp.calls[lights_key]
        rays, traced = S.shadow_rays(inp.positions[src], inp.nrm, inp.hit, lights)
        occluded = oracle(kind, rays, any_hit=True)["prim_id"] >= 0
        assert not occluded[~traced].any()   # the placeholder never reports a hit
        return (~(traced & occluded)).astype(np.uint8), traced, rays
    return cached(("shadow", kind, src, lights_key), make)


def upload_shadow_inputs(ctx, dev):
    inp = shadow_inputs()
    return {SRC_RAY32: (dev.put(inp.rays), dev.put(inp.rec32)), SRC_HOST44: (dev.put(inp.hrays), dev.put(inp.rec44)),
            SRC_GRID: (None, dev.put(inp.grid32))}


def cast_shadow_source(ctx, dev, bufs, src, lights):
    d_mask = dev.alloc(N * len(lights))
    d_rays, d_recs = bufs[src]
    if src == SRC_GRID:
        ctx.cast_grid_shadows(capi.camera_look(CAM[0], CAM[1], W, H, CAM[2]), W, H, d_recs, lights, d_mask)
    else:
        ctx.cast_shadows(d_rays, d_recs, N, lights, d_mask, flags=capi.FLAG_HOST_LAYOUT if src == SRC_HOST44 else 0)
    return dev.get(d_mask, N * len(lights), np.uint8), ctx.last_kernel_variant()


def check_shadow_calls(kind, kernel, lights_keys, variant):
    """Every source layout, every call of `lights_keys`: the mask against the oracle's, byte for byte; pairs without a ray read 1."""
    sc, inp = scene(kind), shadow_inputs()
    ctx = capi.Context(0, kernel=kernel)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        bufs = upload_shadow_inputs(ctx, dev)
        for key in lights_keys:
            lights = inp.four if key == "four" else inp.calls[key]
            for src in (SRC_RAY32, SRC_HOST44, SRC_GRID):
                want, traced, _ = shadow_expected(kind, src, key)
                got, name = cast_shadow_source(ctx, dev, bufs, src, lights)
                assert name.startswith(variant(src)), (name, variant(src))
                assert (got[~traced] == 1).all(), "a pair without a ray (miss, light off, dist < 1e-6) must read 1"
                np.testing.assert_array_equal(got, want, err_msg="%s source %d lights %s" % (kind, src, key))
    finally:
        dev.free()
        ctx.close()


def test_edge_pairs_reach_what_they_are_made_for():
    """(CPU arithmetic only.)  The expected masks hold shadowed and lit pairs, pairs without a ray of all three kinds, rays with an infinite
    t_max, zero directions and origins at 1e30; the sources' positions agree where they must."""
    inp = shadow_inputs()
    np.testing.assert_array_equal(inp.positions[SRC_RAY32][inp.hit], inp.pos[inp.hit])   # 0 + p * 1 is p (-0.0 comes back +0.0)
    for key in (0, 1):
        m32, t32, r32 = shadow_expected("room", SRC_RAY32, key)
        m44, t44, r44 = shadow_expected("room", SRC_HOST44, key)
        np.testing.assert_array_equal(m32, m44)
        np.testing.assert_array_equal(t32, t44)
        assert m44.min() == 0 and m44.max() == 1
        lit_without_ray = ~t44.reshape(16, N)
        assert lit_without_ray[15].all()                                      # cast_shadows == 0
        assert lit_without_ray[:, ~inp.hit].all()                             # misses
        assert key != 0 or lit_without_ray[:15][:, inp.hit].any()             # dist < 1e-6: among the lights of the first call
    _, t0, r0 = shadow_expected("room", SRC_HOST44, 0)
    live = r0[t0]
    assert (live["t_max"] == S.MIN_DIST).any() and np.isinf(live["t_max"]).any() and (np.abs(live["origin"]) >= 1e30).any()
    _, t1, r1 = shadow_expected("room", SRC_HOST44, 1)
    assert ((r1[t1]["direction"] == 0).all(axis=1)).any()
    _, tg, rg = shadow_expected("room", SRC_GRID, 0)
    assert (rg[tg]["t_max"] == S.MIN_DIST).any()                              # the grid source reaches the threshold too (t = 0, n = 0)


@pytest.mark.parametrize("kind", ["room", "room_tl"])
def test_shadow_edges_in_the_plain_kernels(built, kind):
    """Four lights (16 384 pairs) take the plain kernel by the policy; the two 16-light calls (65 536 pairs each) take it forced."""
    check_shadow_calls(kind, capi.KERNEL_AUTO, ["four"], lambda src: PLAIN[kind] % src)
    check_shadow_calls(kind, capi.KERNEL_LANE, [0, 1], lambda src: PLAIN[kind] % src)


@pytest.mark.parametrize("kind, kernel, width", [("room", capi.KERNEL_AUTO, 8), ("room", capi.KERNEL_LANE4_PERSISTENT, 4),
                                                 ("room", capi.KERNEL_LANE_PERSISTENT, 2), ("room_tl", capi.KERNEL_AUTO, 8)],
                         ids=["flat-auto8", "flat-lane4p", "flat-lane2p", "two-level-auto"])
def test_shadow_edges_in_the_persistent_kernels(built, kind, kernel, width):
    """4 096 records x 16 lights = 65 536 pairs, the smallest batch the policy sends to the persistent kernels: the masks of the plain
    kernel (the test above holds them to the same expected bytes) from every persistent form."""
    tl = "true" if kind == "room_tl" else "false"
    check_shadow_calls(kind, kernel, [0, 1], lambda src: PERSISTENT % (src, width, tl))


# ---- non-finite lights: shadow_invalid accepts them, as the reference does; the derived ray is a NaN ray

def non_finite_lights():
    inp = shadow_inputs()
    L = inp.calls[0][[11, 11, 12, 11, 13]].copy()
    L["type"], L["cast_shadows"] = T.LIGHT_POINT, 1
    L["position"] = [(1.0, -1.75, 1.5), (np.nan, 2.0, 1.0), (-3.0, -2.25, -3.0), (np.inf, 3.0, 0.0), (0.5, -2.25, 0.5)]
    L["type"][2] = T.LIGHT_SPOT
    return L, np.array([True, False, True, False, True])


def non_finite_expected(kind):
    def make():
        inp = shadow_inputs()
        L, ordinary = non_finite_lights()
        rays, traced = S.shadow_rays(inp.pos, inp.nrm, inp.hit, L)
        occluded = oracle(kind, rays, any_hit=True)["prim_id"] >= 0
        return (~(traced & occluded)).astype(np.uint8), traced, rays
    return cached(("non-finite", kind), make)


@pytest.mark.parametrize("kind, tile", [("room", 1), ("room_tl", 1), ("room", 4)], ids=["flat-plain", "two-level-plain", "flat-persistent"])
def test_non_finite_lights_leave_the_other_lights_alone(built, kind, tile):
    """One light with a NaN component and one at +inf among three ordinary ones.  The pairs of the ordinary lights equal those of a call
    without the other two; the pairs of the non-finite lights equal what the oracle gives for the restated (NaN) rays: lit, every one
    (test_shadow_cpu.py's sibling check on the CPU: the oracle's walk and its brute-force loop agree on them)."""
    sc, inp = scene(kind), shadow_inputs()
    L, ordinary = non_finite_lights()
    want, traced, rays = non_finite_expected(kind)
    want, traced = want.reshape(5, N), traced.reshape(5, N)
    assert np.isnan(rays.reshape(5, N)["direction"][1][traced[1]]).any() and np.isnan(rays.reshape(5, N)["direction"][3][traced[3]]).any()
    assert (want[~ordinary] == 1).all() and want[ordinary].min() == 0
    n = N * tile
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        d_rays, d_recs = dev.put(np.tile(inp.hrays, tile)), dev.put(np.tile(inp.rec44, tile))
        d_all, d_some = dev.alloc(5 * n), dev.alloc(3 * n)
        ctx.cast_shadows(d_rays, d_recs, n, L, d_all, flags=capi.FLAG_HOST_LAYOUT)
        name = ctx.last_kernel_variant()
        assert ("persistent" in name) == (tile > 1), name
        ctx.cast_shadows(d_rays, d_recs, n, L[ordinary], d_some, flags=capi.FLAG_HOST_LAYOUT)
        got, some = dev.get(d_all, 5 * n, np.uint8).reshape(5, n), dev.get(d_some, 3 * n, np.uint8).reshape(3, n)
        np.testing.assert_array_equal(got[ordinary], some)
        np.testing.assert_array_equal(got, np.tile(want, (1, tile)))
    finally:
        dev.free()
        ctx.close()


# ------------------------------------------------------------------------------------------------------------ reflections

class ReflectionInputs:
    def __init__(self):
        self.d, self.n, self.pos, self.hit, self.select = E.reflection_records()
        # mrt_hit32 + rays from an array: o = position, t = 0 (o + d * 0 is o); the incoming direction is the ray's
        self.rays = E.rays32(self.pos, self.d)
        self.rec32 = E.records32(self.n, self.hit, np.zeros(N, dtype=F))
        self.hrays = po.make_host_rays(self.rays)
        self.rec44 = E.records44(self.pos, self.n, self.hit)
        self.traced = self.hit & (self.select != 0)
        self.want_rays, self.flipped = R.reflection_rays(self.d, hit_point(self.rays, np.zeros(N, dtype=F)), self.n, self.traced, MAX_DIST)
        same(self.want_rays, R.reflection_rays(self.d, self.pos, self.n, self.traced, MAX_DIST)[0])   # both layouts: the same rays
        self.host_want_rays = po.make_host_rays(self.want_rays)


def reflection_inputs():
    return cached("reflection_inputs", ReflectionInputs)


def reflection_expected(kind):
    return cached(("reflection", kind), lambda: oracle(kind, reflection_inputs().want_rays))


def chained_lights():
    L = np.zeros(2, dtype=T.LIGHT)
    L["cast_shadows"] = 1
    L[0]["type"], L[0]["position"] = T.LIGHT_POINT, (1.0, 4.5 - E.LOWER, 1.5)
    L[1]["type"], L[1]["direction"] = T.LIGHT_DIRECTIONAL, (0.3, 1.0, 0.2)
    return L


def chained_expected(kind):
    """the lit mask of a shadow cast on the reflected records and rays"""
    def make():
        inp, hits = reflection_inputs(), reflection_expected(kind)
        srays, traced = S.shadow_rays(hit_point(inp.want_rays, hits["t"]), hits["normal"], hits["prim_id"] != -1, chained_lights())
        return (~(traced & (oracle(kind, srays, any_hit=True)["prim_id"] >= 0))).astype(np.uint8)
    return cached(("chained", kind), make)


def test_reflection_records_reach_what_they_are_made_for():
    """(CPU arithmetic only.)"""
    inp = reflection_inputs()
    t = inp.traced
    assert inp.flipped.any() and (~inp.flipped[t]).any()                                       # back and front faces
    assert set(inp.select[inp.hit]) == {0, 1, 2, 255} and (inp.select[~inp.hit] != 0).any()   # both reasons for no ray, and both at once
    assert t[inp.select >= 2].any()                                                             # any nonzero byte traces
    same(inp.want_rays[~t], np.repeat(R.PLACEHOLDER, (~t).sum()))
    d = inp.want_rays["direction"][t]
    assert (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any() and ((d != 0) & (np.abs(d) < F(1e-9))).any()
    inv, big = inp.host_want_rays["inv_direction"][t], F(1) / F(1e-9)
    assert (inv[np.abs(d) < F(1e-9)] == np.where(d[np.abs(d) < F(1e-9)] < 0, -big, big)).all()
    assert (np.abs(d) > 1e17).any()                                                             # |d| = 1e18 comes through unnormalised
    for kind in ("room", "room_tl"):
        hits = reflection_expected(kind)
        assert (hits["prim_id"][t] != -1).any() and (hits["prim_id"][t] == -1).any()
        same(hits[~t], np.repeat(R.PLACEHOLDER_HIT, (~t).sum()))
        m = chained_expected(kind)
        assert m.min() == 0 and m.max() == 1


@pytest.mark.parametrize("kind, tile, variant", [("room", 1, "trace_reflection_lane_kernel<%d>"),
                                                 ("room_tl", 1, "trace_reflection_two_level_kernel<%d>"),
                                                 ("room", 16, "trace_reflection_persistent_kernel<%d, 8, false>"),
                                                 ("room_tl", 16, "trace_reflection_persistent_kernel<%d, 8, true>")],
                         ids=["flat-plain", "two-level-plain", "flat-persistent", "two-level-persistent"])
def test_reflection_edges(built, kind, tile, variant):
    """The hand-made records (tiled to 65 536 for the persistent forms) in both layouts: output records and output rays against the
    restatement traced by the oracle, byte for byte -- in the 60-byte layout with inv_direction and dir_sign as Ray::_precompute fills
    them -- and one shadow cast chained on the outputs of each layout."""
    sc, inp = scene(kind), reflection_inputs()
    want, n = np.tile(reflection_expected(kind), tile), N * tile
    want_rays, host_want_rays = np.tile(inp.want_rays, tile), np.tile(inp.host_want_rays, tile)
    lights, want_mask = chained_lights(), np.tile(chained_expected(kind).reshape(2, N), (1, tile)).reshape(-1)
    ctx = capi.Context(0)
    dev = Dev(ctx)
    try:
        sc.upload(ctx)
        d_sel = dev.put(np.tile(inp.select, tile))
        # mrt_ray32 / mrt_hit32
        d_rays, d_recs = dev.put(np.tile(inp.rays, tile)), dev.put(np.tile(inp.rec32, tile))
        d_out, d_orays = dev.alloc(n * 32), dev.alloc(n * 32)
        ctx.cast_reflections(d_rays, d_recs, n, d_out, MAX_DIST, d_select=d_sel, d_out_rays=d_orays)
        assert ctx.last_kernel_variant() == variant % 4, ctx.last_kernel_variant()
        same(dev.get(d_orays, n, T.RAY32), want_rays, "rays")
        same(dev.get(d_out, n, T.HIT32), want, "records")
        d_mask = dev.alloc(2 * n)
        ctx.cast_shadows(d_orays, d_out, n, lights, d_mask)
        np.testing.assert_array_equal(dev.get(d_mask, 2 * n, np.uint8), want_mask)
        # mrt_host_ray60 / mrt_host_hit44
        d_hr, d_r44 = dev.put(np.tile(inp.hrays, tile)), dev.put(np.tile(inp.rec44, tile))
        d_o44, d_or60 = dev.alloc(n * 44), dev.alloc(n * 60)
        ctx.cast_reflections(d_hr, d_r44, n, d_o44, MAX_DIST, d_select=d_sel, d_out_rays=d_or60, flags=capi.FLAG_HOST_LAYOUT)
        assert ctx.last_kernel_variant() == variant % 5, ctx.last_kernel_variant()
        same(dev.get(d_or60, n, T.HOST_RAY60), host_want_rays, "host rays")
        same(dev.get(d_o44, n, T.HOST_HIT44), po.unpack_hits(want, host_want_rays), "host records")
        d_mask44 = dev.alloc(2 * n)
        ctx.cast_shadows(d_or60, d_o44, n, lights, d_mask44, flags=capi.FLAG_HOST_LAYOUT)
        np.testing.assert_array_equal(dev.get(d_mask44, 2 * n, np.uint8), want_mask)
    finally:
        dev.free()
        ctx.close()
