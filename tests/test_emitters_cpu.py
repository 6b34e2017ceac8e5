"""Emissive triangles as light sources without a device: the numpy restatement (messyerraytracer_amd/emitters.py) held to what
include/mrt_hip.h promises of it -- the table for 0, 1 and all-emissive inputs and what it leaves out, the range of its total, a strictly
increasing CDF; a selection whose histogram is the table's exact pmf; points uniform on the triangle; the diffuse term against an fp64
quadrature; and the acceptance test of the estimator's split: the numpy frame loop on synth.room() with an emissive ceiling patch and
no analytic lights gives, with and without emitter sampling, the same block means within their errors.  The emitter scenes of
test_emitters_gpu.py are made here, with the CPU-side proof that the oracle's two any-hit answers (the walk and brute force) disagree
on far fewer than 1 % of their shadow rays.  The host-only units run as programs of their own."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from messyerraytracer_amd import bounce as B
from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi, synth, types as T
from messyerraytracer_amd import emitters as E
from messyerraytracer_amd import hemisphere as H
from messyerraytracer_amd import path as P
from messyerraytracer_amd import surface as S
from oracle import pyoracle as po

F = np.float32
ROOM_CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
SOUP_CAM = ((0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0)
CEILING0, CELLS = 1682, 29          # synth.room(): the ceiling's first triangle, cells per side (two triangles per cell)
PATCH = (10, 19)                    # the emissive ceiling patch: cells [10, 19) x [10, 19), 162 triangles, about 3.1 m square


def materials():
    m = np.zeros(4, T.MATERIAL)
    m["albedo"], m["roughness"], m["specular"] = ((0.7, 0.7, 0.7), (0.8, 0.6, 0.4), (0.5, 0.5, 0.9), (0.9, 0.9, 0.9)), 0.6, 0.5
    m["metallic"] = (0.0, 0.0, 0.2, 0.0)
    m["emission"] = ((0, 0, 0), (1.0, 0.9, 0.7), (0.2, 0.5, 1.0), (1.0, 1.0, 1.0))
    m["emission_energy"] = (0.0, 8.0, 3.0, -2.0)       # 1, 2: emitters; 3: a colour with an energy below 0
    return m


def patch_ids(n_flat, value=1):
    ids = np.zeros(n_flat, np.uint32)
    for i in range(*PATCH):
        for j in range(*PATCH):
            c = CEILING0 + 2 * (i * CELLS + j)
            ids[c:c + 2] = value
    return ids


@functools.lru_cache(maxsize=None)
def emitter_scene(kind):
    """(world-space vertices [n, 3, 3], layers [n], camera, ShadeData) of the scenes the emitter tests share.  room / room_tl: synth.room()
    flat, the ceiling patch on material 1 and every 97th triangle (walls, sphere, boxes) on material 2; soup: every 7th triangle of
    synth.soup(2000, 0.4, 3) on material 1 or 2, every 11th on material 3 (a colour without energy)."""
    if kind == "soup":
        verts = synth.soup(2000, 0.4, 3)
        n = verts.shape[0]
        layers, cam = np.full(n, 0xFFFFFFFF, np.uint32), SOUP_CAM
        ids = np.zeros(n, np.uint32)
        ids[::11] = 3
        ids[::7] = 1 + (np.arange(0, n, 7) // 7) % 2
    else:
        local, inst = synth.room()
        verts = synth.flatten_instances(local, inst)
        n = verts.shape[0]
        layers, cam = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32), ROOM_CAM
        ids = patch_ids(n)
        ids[5::97] = 2
    return verts, layers, cam, S.ShadeData(n, materials(), ids)


def world_tris(verts, layers):
    return po.make_triangles(verts, None, layers)


def test_exports_and_sizes():
    L = capi.load()
    for s in ("mrt_build_emitters", "mrt_clear_emitters", "mrt_emitter_info", "mrt_emitter_table", "mrt_cast_emitter_shadows",
              "mrt_cast_grid_emitter_shadows", "mrt_light_emitter_surfaces", "mrt_light_grid_emitter_surfaces", "mrt_path_step_emitters",
              "mrt_path_grid_step_emitters"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert L.mrt_struct_size(capi.STRUCT_EMITTER_SELECT) == C.sizeof(capi.EmitterSelect) == T.EMITTER_SELECT.itemsize == 24
    assert L.mrt_struct_size(capi.STRUCT_EMITTER64) == T.EMITTER64.itemsize == 64
    assert L.mrt_struct_size(35) == 0 and L.mrt_struct_size(37) == 0 and L.mrt_struct_size(39) == 0
    assert L.mrt_struct_size(capi.STRUCT_LIGHT_SELECT) == 24                             # the struct before them is as it was
    # clear of the bounce's draws (<= 129) and of the light-selecting draws (256 .. 288)
    assert T.path_emitter_draw(0) == 512 and T.path_emitter_draw(32) + 2 == 642 and T.path_select_draw(32) < 512
    assert P.first_draw(32) + 3 < 256
    P_ = C.c_void_p(16)  # never dereferenced: a null context fails first
    d, o = capi.EmitterSelect(0, 512, None, 16), capi.LightOut(16)
    cam = capi.camera_look((0, 0, 3), (0, 0, -1), 4, 4, 60.0)
    assert L.mrt_build_emitters(None, P_, 4, 0) == capi.ERR_INVALID and L.mrt_clear_emitters(None) == capi.ERR_INVALID
    assert L.mrt_emitter_info(None, None, None) == capi.ERR_INVALID and L.mrt_emitter_table(None, P_, P_, 4) == capi.ERR_INVALID
    assert L.mrt_cast_emitter_shadows(None, P_, P_, 4, C.byref(d), P_, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    assert L.mrt_cast_grid_emitter_shadows(None, C.byref(cam), 4, 4, 0, 4, P_, C.byref(d), P_, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    assert L.mrt_light_emitter_surfaces(None, P_, P_, P_, 4, C.byref(d), None, 0, C.byref(o), 0) == capi.ERR_INVALID
    assert L.mrt_light_grid_emitter_surfaces(None, C.byref(cam), 4, 4, 0, 4, P_, P_, C.byref(d), None, 0, C.byref(o), 0) == capi.ERR_INVALID
    assert L.mrt_path_step_emitters(None, P_, P_, P_, 4, None, None, 0) == capi.ERR_INVALID
    assert L.mrt_path_grid_step_emitters(None, C.byref(cam), 4, 4, 0, 4, P_, P_, None, None, 0) == capi.ERR_INVALID


# ---- the table -----------------------------------------------------------------------------------------------------------------------

def random_tris(n, seed=1):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-4, 4, (n, 1, 3)) + rng.uniform(-0.5, 0.5, (n, 3, 3))
    return po.make_triangles(v.astype(F), None, None)


def check_table(rows, cdf, n_emit):
    assert rows.shape[0] == cdf.shape[0] == n_emit
    if n_emit == 0:
        return
    q = rows["q"].astype(np.int64)
    assert (q >= 1).all()
    np.testing.assert_array_equal(np.cumsum(q), cdf.astype(np.int64))
    assert (np.diff(cdf.astype(np.int64)) > 0).all()                                  # strictly increasing
    total = int(cdf[-1])
    assert 2 ** 31 - n_emit < total <= 2 ** 31, total


def test_table_for_no_one_and_every_emitter():
    tris = random_tris(300)
    m = materials()
    for n_tris in (1, 2, 300):
        t = tris[:n_tris]
        assert E.build_table(t, None)[0].shape[0] == 0                                 # no shade data resident
        assert E.build_table(t, S.ShadeData(n_tris, m, np.zeros(n_tris, np.uint32)))[0].shape[0] == 0
        assert E.build_table(t, S.ShadeData(n_tris, m[:0], np.ones(n_tris, np.uint32)))[0].shape[0] == 0
        one = np.zeros(n_tris, np.uint32)
        one[n_tris // 2] = 2
        rows, cdf = E.build_table(t, S.ShadeData(n_tris, m, one))
        check_table(rows, cdf, 1)
        assert rows["q"][0] == cdf[0] == 2 ** 31 and rows["prim_id"][0] == n_tris // 2 and rows["material"][0] == 2
        np.testing.assert_array_equal(rows["radiance"][0], m["emission"][2] * F(3.0))
        rows, cdf = E.build_table(t, S.ShadeData(n_tris, m, 1 + np.arange(n_tris, dtype=np.uint32) % 2))
        check_table(rows, cdf, n_tris)
        np.testing.assert_array_equal(rows["prim_id"], np.arange(n_tris))              # input order
        np.testing.assert_array_equal(rows["v0"], t["v0"])
        # larger weights get larger integers, and the largest within rounding of its share
        _, area, w, _ = E.triangle_weights(t, S.ShadeData(n_tris, m, 1 + np.arange(n_tris, dtype=np.uint32) % 2))
        order = np.argsort(w, kind="stable")
        assert (np.diff(rows["q"][order].astype(np.int64)) >= 0).all()
        share = w.astype(np.float64) / w.astype(np.float64).sum()
        assert np.abs(rows["q"] / 2.0 ** 31 - share).max() < 2.0 ** -20 * n_tris + 1e-6


def test_table_leaves_out_what_cannot_emit():
    """Zero-area triangles, ids out of range (the triangle's and the material's), emission_energy <= 0, a weight that is not finite."""
    n = 64
    tris = random_tris(n)
    ids = np.ones(n, np.uint32)
    tris["edge2"][3] = tris["edge1"][3] * F(2)                                        # zero area
    tris["edge1"][4] = 0
    tris["id"][5] = n                                                                   # past the shade data's n_tris
    tris["id"][6] = 0xFFFFFFFF
    ids[7] = 4                                                                          # past the materials
    ids[8] = 0                                                                          # energy 0
    ids[9] = 3                                                                          # energy < 0 with a colour
    tris["edge1"][10] = F(3e38)                                                         # an infinite area
    tris["edge1"][11, 0] = np.nan
    rows, cdf = E.build_table(tris, S.ShadeData(n, materials(), ids))
    check_table(rows, cdf, n - 9)
    assert not set(range(3, 12)) & set(rows["prim_id"].tolist())
    _, area, w, _ = E.triangle_weights(tris, S.ShadeData(n, materials(), ids))
    assert area[3] == 0 and area[4] == 0 and not np.isfinite(area[10]) and (w[3:12] == 0).all()
    # the triangle's id indexes the material ids, not its place in the array
    swapped = tris.copy()
    swapped["id"][[0, 8]] = 8, 0
    r2, _ = E.build_table(swapped, S.ShadeData(n, materials(), ids))
    assert 8 not in r2["prim_id"][:1] and r2["prim_id"][0] == 1 and (r2["prim_id"] == 0).sum() == 1


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 1 << 17, T.MAX_EMITTERS])
def test_total_range_and_strict_cdf_over_weights_spanning_2_20(n):
    rng = np.random.default_rng(n)
    w = (2.0 ** rng.uniform(0, 20, n)).astype(F)
    q, cdf = E.integer_weights(w)
    rows = np.zeros(n, T.EMITTER64)
    rows["q"] = q
    check_table(rows, cdf, n)
    # equal weights: every q the same, the total as close to 2^31 as n allows
    q, cdf = E.integer_weights(np.full(n, 0.37, F))
    assert (q == q[0]).all() and 2 ** 31 - n < int(cdf[-1]) <= 2 ** 31


# ---- the selection and the point ------------------------------------------------------------------------------------------------------

N_SEL = 65536


def stream_words(draw, frame=3):
    return B.draw(P.stream_seed(np.arange(N_SEL, dtype=np.uint64), frame), draw)


@pytest.mark.parametrize("n", [3, 1000, 1 << 17])
def test_selection_follows_the_exact_pmf(n):
    """65 536 selections from the stream's own words against q / 2^31, the probabilities being exact sums of integers: each count of
    the histogram within 5 binomial standard deviations of its expectation.  The histogram's bins: every entry whose expected count is
    at least 25 (where a binomial count is near enough to normal for a bound in standard deviations to mean what it says: its skewness
    is below 0.2), all the rarer entries pooled into one bin (a single entry expected 0.03 times is drawn once with probability 3 %,
    which is 5.7 of its standard deviations: with weights spanning 2^20 hundreds of entries are that rare, and some are drawn); 64
    bins of consecutive entries; the small and the large half by weight; and the records left without an emitter."""
    rng = np.random.default_rng(50 + n)
    w = (2.0 ** rng.uniform(0, 20, n)).astype(F)
    if n == 3:
        w = np.array([1.0, 2.0 ** 10, 2.0 ** 20], F)
    q, cdf = E.integer_weights(w)
    k = E.select_emitters(cdf, stream_words(T.path_emitter_draw(1)))
    none = k == T.EMITTER_NONE
    assert (k[~none] < n).all()
    counts = np.bincount(k[~none], minlength=n).astype(np.float64)
    q = q.astype(np.float64)

    def within(count, prob):
        sd = np.sqrt(N_SEL * prob * (1 - prob))
        assert (np.abs(count - N_SEL * prob) <= 5 * sd + 1e-9).all(), (count, N_SEL * prob, sd)

    common = N_SEL * q / 2.0 ** 31 >= 25
    within(counts[common], q[common] / 2.0 ** 31)
    within(np.array([counts[~common].sum()]), np.array([q[~common].sum()]) / 2.0 ** 31)
    assert n != 1000 or common.sum() > 100
    bins = np.minimum(np.arange(n) * 64 // n, 63)
    within(np.bincount(bins, counts, 64)[:min(n, 64)], np.bincount(bins, q, 64)[:min(n, 64)] / 2.0 ** 31)
    small = q <= np.median(q)
    within(np.array([counts[small].sum(), counts[~small].sum()]), np.array([q[small].sum(), q[~small].sum()]) / 2.0 ** 31)
    within(np.array([none.sum()]), np.array([1 - cdf[-1] / 2.0 ** 31]))
    # a mapping of word * total >> 32 would not: the pmf here is exact, so the first entry above a target is the whole rule
    t = np.array([0, int(cdf[0]) - 1, int(cdf[0]), int(cdf[-1]) - 1], np.uint64)
    np.testing.assert_array_equal(E.select_emitters(cdf, (t << np.uint64(1)).astype(np.uint32) | np.uint32(1)), [0, 0, 1, n - 1])
    if cdf[-1] < 2 ** 31:
        assert E.select_emitters(cdf, np.array([(int(cdf[-1]) << 1) & 0xFFFFFFFF], np.uint32))[0] == T.EMITTER_NONE
    assert (E.select_emitters(np.zeros(0, np.uint32), stream_words(512)) == T.EMITTER_NONE).all()


def test_points_are_uniform_on_the_triangle():
    """a and b of 65 536 points from the stream's draws: mean 1/3 each within 5 standard errors; so is 1 - a - b; all inside."""
    a, b = E.triangle_point(H.to_float(stream_words(T.path_emitter_draw(0) + 1)), H.to_float(stream_words(T.path_emitter_draw(0) + 2)))
    for x in (a.astype(np.float64), b.astype(np.float64), 1.0 - a.astype(np.float64) - b):
        assert abs(x.mean() - 1 / 3) <= 5 * x.std(ddof=1) / np.sqrt(N_SEL), (x.mean(), x.std())
        assert abs(x.var() - 1 / 18) < 0.002                                            # the variance of a barycentric coordinate
    assert (a >= 0).all() and (b >= 0).all() and (a + b <= F(1) + F(1e-6)).all()
    # uniform in area: a quarter of the points in each of the four congruent sub-triangles
    part = np.where(a > 0.5, 0, np.where(b > 0.5, 1, np.where(a + b < 0.5, 2, 3)))
    c = np.bincount(part, minlength=4)
    assert (np.abs(c - N_SEL / 4) <= 5 * np.sqrt(N_SEL * 0.25 * 0.75)).all(), c


# ---- the diffuse term -------------------------------------------------------------------------------------------------------------------

def lamp_and_floor():
    """A two-triangle lamp (materials 1 and 2, unequal areas) 3 m above hand-made floor rows that nothing occludes."""
    quad = np.array([[[-1.0, 3.0, -0.5], [1.0, 3.0, -0.5], [1.0, 3.0, 0.7]], [[-1.0, 3.0, -0.5], [1.0, 3.0, 0.7], [-0.6, 3.2, 0.7]]], F)
    tris = po.make_triangles(quad, None, None)
    shade = S.ShadeData(2, materials(), np.array([1, 2], np.uint32))
    rng = np.random.default_rng(9)
    n = 12
    pos = np.stack([rng.uniform(-2.5, 2.5, n), np.zeros(n), rng.uniform(-2.5, 2.5, n)], axis=1).astype(F)
    nrm = np.tile(np.array([0, 1, 0], F), (n, 1))
    nrm[n // 2:] = B.normalized((nrm[n // 2:] + rng.uniform(-0.4, 0.4, (n - n // 2, 3))).astype(F))
    d = B.normalized((pos - np.array([0.0, 2.0, 5.0], F)).astype(F))
    rows = np.zeros(n, T.SURFACE64)
    rows["normal"], rows["albedo"], rows["metallic"], rows["roughness"], rows["specular"] = nrm, rng.uniform(0.2, 0.9, (n, 3)), 0.25, 0.5, 0.5
    rows["n_dot_v"] = 0.5
    return tris, shade, rows, pos, nrm, d


def quadrature(tris, le, rows, pos, nrm, d, side=128):
    """fp64, side^2 = 2^14 stratified points per triangle (cell midpoints through the area-preserving map of the sampler):
    (diff / pi) * Le * integral of max(n . w, 0) |ng . w| / r^2 dA."""
    k = (np.arange(side) + 0.5) / side
    u1, u2 = np.meshgrid(k, k, indexing="ij")
    su = np.sqrt(u1).ravel()
    a, b = su * (1 - u2.ravel()), su * u2.ravel()
    n = nrm.astype(np.float64).copy()
    n[(n * d.astype(np.float64)).sum(axis=1) > 0] *= -1
    org = pos.astype(np.float64) + n * 1e-3
    diff = rows["albedo"].astype(np.float64) * (1 - rows["metallic"].astype(np.float64))[:, None]
    out = np.zeros((pos.shape[0], 3))
    for t in range(tris.shape[0]):
        v0, e1, e2 = (tris[f][t].astype(np.float64) for f in ("v0", "edge1", "edge2"))
        c = np.cross(e1, e2)
        area, ng = 0.5 * np.linalg.norm(c), c / np.linalg.norm(c)
        y = v0 + a[:, None] * e1 + b[:, None] * e2
        to = y[None, :, :] - org[:, None, :]
        r2 = (to * to).sum(axis=2)
        w = to / np.sqrt(r2)[:, :, None]
        g = np.maximum((w * n[:, None, :]).sum(axis=2), 0) * np.abs(w @ ng) / r2
        out += (diff / np.pi) * le[t].astype(np.float64) * (g.mean(axis=1) * area)[:, None]
    return out


def test_diffuse_term_against_an_fp64_quadrature():
    """The mean of the term over F = 4096 frames within 5 s / sqrt(F) of the quadrature, s the sample deviation, per record and channel."""
    tris, shade, rows, pos, nrm, d = lamp_and_floor()
    table = E.build_table(tris, shade)
    assert table[0].shape[0] == 2
    frames, n = 4096, rows.shape[0]
    pix = E.frame_pixels(np.arange(n, dtype=np.uint64), range(frames))
    rep = lambda x: np.tile(x, (frames,) + (1,) * (x.ndim - 1))
    s = E.emitter_samples(rep(d), rep(pos), rep(nrm), np.ones(n * frames, bool), pix, 0, T.path_emitter_draw(0), *table)
    assert s["traced"].mean() > 0.9 and len(np.unique(s["emitter"])) >= 2
    term = E.emitter_terms(rep(rows), s).astype(np.float64).reshape(frames, n, 3)
    want = quadrature(tris, table[0]["radiance"], rows, pos, nrm, d)
    mean, sd = term.mean(axis=0), term.std(axis=0, ddof=1)
    assert (want > 0).all() and (np.abs(mean - want) <= 5 * sd / np.sqrt(frames)).all(), np.abs(mean - want) / (sd / np.sqrt(frames))
    # the frames trick draws what the frames draw
    one = E.emitter_samples(d, pos, nrm, np.ones(n, bool), np.arange(n, dtype=np.uint64), 77, T.path_emitter_draw(0), *table)
    np.testing.assert_array_equal(one["rays"], s["rays"][77 * n:78 * n])
    # written and accumulated forms, the mask, a miss
    hit = np.arange(n) % 5 != 4
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    o = E.emitter_direct(rows, hit, one, mask)
    assert (o[~hit] == 0).all() and (o[hit, 3] == 1).all() and (o[hit & (mask == 0), :3] == 0).all() and (o[hit & (mask != 0) & one["traced"], :3] > 0).all()
    base = np.full((n, 4), 0.25, F)
    acc = E.emitter_direct(rows, hit, one, mask, base)
    np.testing.assert_array_equal(acc[~hit], base[~hit])
    np.testing.assert_array_equal(acc[hit, :3], F(0.25) + o[hit, :3])
    assert (acc[:, 3] == F(0.25)).all()


# ---- the split is consistent: the acceptance test ----------------------------------------------------------------------------------------

W, H_, BLOCK, BOUNCES = 32, 24, 8, 3
FRAMES = 64   # the smallest power of two at which the loop WITHOUT sampling has a relative standard error below 10 % on every block


def block_means(state, frames):
    lum = state["radiance"].astype(np.float64).sum(axis=1).reshape(frames, H_ // BLOCK, BLOCK, W // BLOCK, BLOCK)
    return lum.mean(axis=(2, 4)).reshape(frames, -1)


def test_the_split_is_consistent_on_the_room():
    """synth.room() at 32 x 24 with the emissive ceiling patch alone (material ids), no analytic light, 3 bounces, the oracle tracing: the
    means over F frames of the 8 x 8 pixel blocks agree, with and without emitter sampling, within 5 standard errors of their
    difference (the errors from the per-frame block means).  F = 64: first, the loop without sampling is below 10 % on every block at
    64 frames and not at 32.  Observed: the largest |difference| is 1.69 standard errors, 0.34 of the bound (1.88 and 0.38 at F = 1024)."""
    verts, layers, cam, _ = emitter_scene("room")
    n_flat = verts.shape[0]
    shade = S.ShadeData(n_flat, materials(), patch_ids(n_flat))
    table = E.build_table(world_tris(verts, layers), shade)
    assert table[0].shape[0] == 2 * (PATCH[1] - PATCH[0]) ** 2
    sc = po.OracleScene(verts, layers=layers)
    rays = np.tile(po.grid_rays(cam[0], cam[1], W, H_, cam[2]), FRAMES)
    pix = E.frame_pixels(np.arange(W * H_, dtype=np.uint64), range(FRAMES))
    env = np.zeros(1, T.ENVIRONMENT)[0]

    def shade_fn(r, hits):
        return S.resolve(r["direction"], hits["normal"], hits["prim_id"] != -1, hits["prim_id"].view(np.uint32), hits["bary_u"], hits["bary_v"], shade)

    def occluded(r, traced):
        return sc.trace(r, any_hit=True)["prim_id"] >= 0

    plain = block_means(E.frame_loop(sc.trace, occluded, rays, shade_fn, env, pix, 0, BOUNCES, None), FRAMES)
    rel = lambda b: (b.std(axis=0, ddof=1) / np.sqrt(b.shape[0])) / b.mean(axis=0)
    assert (rel(plain) < 0.10).all(), rel(plain)
    assert not (rel(plain[:FRAMES // 2]) < 0.10).all()                                   # F is the smallest such power of two
    nee = block_means(E.frame_loop(sc.trace, occluded, rays, shade_fn, env, pix, 0, BOUNCES, table), FRAMES)
    diff = plain.mean(axis=0) - nee.mean(axis=0)
    se = np.sqrt(plain.var(axis=0, ddof=1) / FRAMES + nee.var(axis=0, ddof=1) / FRAMES)
    print("block |difference| / standard error:", np.round(np.abs(diff) / se, 2), "largest ratio to the bound:", (np.abs(diff) / se).max() / 5)
    assert (np.abs(diff) <= 5 * se).all(), diff / se
    assert (rel(nee) < rel(plain)).all()                                                 # and the sampling is what it is for


@pytest.mark.parametrize("kind", ["room", "soup"])
def test_the_oracle_alone_agrees_with_itself_on_the_shadow_rays(kind):
    """The placement test_emitters_gpu.py checks mask bytes on: the oracle's walk and its brute force disagree on at most 1 % of the
    emitter shadow rays of a 64 x 64 grid (they leave those records out)."""
    verts, layers, cam, shade = emitter_scene(kind)
    table = E.build_table(world_tris(verts, layers), shade)
    assert table[0].shape[0] > 100 and len(np.unique(table[0]["material"])) == 2
    sc = po.OracleScene(verts, layers=layers)
    rays = po.grid_rays(cam[0], cam[1], 64, 64, cam[2])
    hits = sc.trace(rays)
    hit = hits["prim_id"] != -1
    pos = rays["origin"] + rays["direction"] * hits["t"][:, None]
    s = E.emitter_samples(rays["direction"], pos, hits["normal"], hit, np.arange(4096, dtype=np.uint64), 5, T.path_emitter_draw(0), *table)
    a = sc.trace(s["rays"], any_hit=True)["prim_id"] >= 0
    b = sc.brute(s["rays"], any_hit=True)["prim_id"] >= 0
    assert s["traced"].sum() > 500 and (s["traced"] & a).any() and (s["traced"] & ~a).any()
    assert (a != b)[s["traced"]].mean() <= 0.01, (a != b)[s["traced"]].mean()
    assert (~s["traced"] & hit & (s["emitter"] != T.EMITTER_NONE)).any()                 # refusals occur


# ---- the host-only units -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True])
def test_emitter_data_driver(sanitize):
    """The argument checks in the header's order and the kernels' arguments, without a device; with and without AddressSanitizer and
    UndefinedBehaviorSanitizer."""
    exe = mbuild.build_emitter_data_test(sanitize=sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_emitter_policy_driver():
    """The two new policy entries get ENTRY_SELECTED_SHADOW's plan for as many records, on every scene kind of the record policy's table."""
    exe = mbuild.build_emitter_policy_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
