"""The G-buffer reflection pass without a device: the library exports the two entry points, the struct's size and layout agree and
the calls refuse a null context; the numpy restatement (messyerraytracer_amd/gbuffer.py, what the GPU tests hold the kernels to byte
for byte) against a second route -- a scalar evaluation that does every operation in float64 and rounds it once to float32, which is
exact for + - * / and sqrt because 53 >= 2 * 24 + 2 -- bit for bit over the edge table (tests/gbuffer_cases.py) and a few thousand
seeded texels; the exact properties of the edge cases; and the host program (csrc/host/gbuffer_data_test.cpp, also under
AddressSanitizer and UndefinedBehaviorSanitizer as a program of its own): every refusal in order, and gbuffer.h's rays and image
pixels bit for bit against the restatement through a file written here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import gbuffer as G
import gbuffer_cases as GC

F = np.float32
D = np.float64


def test_exports_sizes_and_layouts():
    L = G.lib()
    for s in ("mrt_cast_gbuffer_reflections", "mrt_reflection_image"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert capi.STRUCT_GBUFFER == 30
    assert L.mrt_struct_size(30) == C.sizeof(G.GBufferDesc) == 160
    assert L.mrt_struct_size(29) == 0 and L.mrt_struct_size(31) == 0
    assert [getattr(G.GBufferDesc, n).offset for n, _ in G.GBufferDesc._fields_] == [0, 4, 8, 72, 136, 140, 144, 152]
    assert L.mrt_struct_size(capi.STRUCT_DENOISE_PARAMS) == 112   # the struct before it is as it was


def test_null_context_is_invalid():
    """(With a context, every bad argument is refused before any device work, in the header's order: test_gbuffer_gpu.py and the host
    program below.)"""
    L = G.lib()
    cam = GC.camera(4, 4)
    g = G.GBuffer(np.zeros(16, F), np.zeros((16, 4), F), cam.inv_projection, cam.inv_view).desc(4096, 8192)
    a, b, c = (C.c_void_p(4096 * k) for k in range(3, 6))
    assert L.mrt_cast_gbuffer_reflections(None, C.byref(g), 4, 4, a, b, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    assert L.mrt_reflection_image(None, C.byref(g), 4, 4, a, b, c, 0) == capi.ERR_INVALID
    assert L.mrt_cast_gbuffer_reflections(None, None, 0, 0, None, None, 0, 0) == capi.ERR_INVALID
    assert L.mrt_reflection_image(None, None, 0, 0, None, None, None, 0) == capi.ERR_INVALID


def test_camera_helper():
    """near maps to depth 0 and far to 1; the float32 inverses are the float64 ones rounded once; a point projects back to its pixel."""
    cam = GC.camera(67, 35)
    fwd = np.asarray(GC.ROOM_FWD) / np.linalg.norm(GC.ROOM_FWD)
    on_axis = cam.origin + fwd * np.array([[GC.NEAR], [GC.FAR], [2.0]])
    d = cam.depth(on_axis)
    assert abs(d[0]) < 1e-12 and abs(d[1] - 1) < 1e-12 and 0 < d[2] < 1
    assert np.array_equal(cam.inv_projection, np.linalg.inv(cam.projection).T.reshape(-1).astype(F))
    assert np.array_equal(cam.inv_view, np.linalg.inv(cam.view).T.reshape(-1).astype(F))
    rays = cam.primary_rays(67, 35)
    p = rays["origin"].astype(D) + rays["direction"].astype(D) * 3.0
    clip = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1) @ (cam.projection @ cam.view).T
    x, y = G._pixels(67, 35)
    np.testing.assert_allclose((clip[:, 0] / clip[:, 3] + 1) / 2 * 67 - 0.5, x, atol=1e-4)
    np.testing.assert_allclose((clip[:, 1] / clip[:, 3] + 1) / 2 * 35 - 0.5, y, atol=1e-4)


# ---- the second route: scalars, every operation in float64 rounded once -----------------------------------------------------------
def _r(x):
    with np.errstate(all="ignore"):
        return F(x)


def _mul(a, b):
    with np.errstate(all="ignore"):
        return _r(D(a) * D(b))


def _add(a, b):
    with np.errstate(all="ignore"):
        return _r(D(a) + D(b))


def _sub(a, b):
    with np.errstate(all="ignore"):
        return _r(D(a) - D(b))


def _div(a, b):
    with np.errstate(all="ignore"):
        return _r(D(a) / D(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return _r(np.sqrt(D(a)))


def _dot3(a, b):
    return _add(_add(_mul(a[0], b[0]), _mul(a[1], b[1])), _mul(a[2], b[2]))


def _normalize(v):
    ln = _sqrt(_dot3(v, v))
    return [_div(c, ln) for c in v]


def _clamp01(x):
    x = x if not (x < F(0)) else F(0)      # max(x, 0) = x < 0 ? 0 : x
    return x if not (F(1) < x) else F(1)   # min(x, 1) = 1 < x ? 1 : x


def _decode(kind, g):
    if kind == G.NORMAL_WORLD:
        return [g[0], g[1], g[2]], g[3]
    fx, fy = _sub(_mul(g[0], F(2)), F(1)), _sub(_mul(g[1], F(2)), F(1))
    z = _sub(_sub(F(1), abs(fx)), abs(fy))
    t = _clamp01(-z)
    nx = _add(fx, -t if fx >= 0 else t)
    ny = _add(fy, -t if fy >= 0 else t)
    return _normalize([nx, ny, z]), g[2]


def second_route(kind, w, h, x, y, thr, depth, g, P, V):
    """(traced, org, dir, d, world, roughness) of one texel"""
    n, rough = _decode(kind, g)
    u, v = _div(_add(F(x), F(0.5)), F(w)), _div(_add(F(y), F(0.5)), F(h))
    cx, cy = _sub(_mul(u, F(2)), F(1)), _sub(_mul(v, F(2)), F(1))
    q = [_add(_add(_add(_mul(P[r], cx), _mul(P[4 + r], cy)), _mul(P[8 + r], depth)), P[12 + r]) for r in range(4)]
    view = [_div(q[0], q[3]), _div(q[1], q[3]), _div(q[2], q[3])]
    world = [_add(_add(_add(_mul(V[r], view[0]), _mul(V[4 + r], view[1])), _mul(V[8 + r], view[2])), V[12 + r]) for r in range(3)]
    d = _normalize([_sub(world[r], V[12 + r]) for r in range(3)])
    k = _mul(F(2), _dot3(n, d))
    dirs = [_sub(d[r], _mul(k, n[r])) for r in range(3)]
    org = [_add(world[r], _mul(n[r], F(0.01))) for r in range(3)]
    traced = bool(depth < F(1)) and bool(rough <= thr) and bool(np.isfinite(org).all()) and bool(np.isfinite(dirs).all())
    return traced, org, dirs, d, world, rough


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def check_table(t, kind):
    rays, traced = G.texel_rays(kind, t["P"], t["V"], t["thr"], GC.MAX_DIST, t["x"], t["y"], t["w"], t["h"], t["depth"], t["guide"])
    n = t["depth"].shape[0]
    hn = np.random.default_rng(5).normal(0, 1, (n, 3)).astype(F)
    img = G.texel_image(kind, t["P"], t["V"], t["thr"], t["x"], t["y"], t["w"], t["h"], t["depth"], t["guide"], np.zeros(n, np.int32), hn)
    for i in range(n):
        tr, org, dirs, d, world, rough = second_route(kind, t["w"][i], t["h"][i], t["x"][i], t["y"][i], t["thr"][i], t["depth"][i],
                                                      t["guide"][i], t["P"][i], t["V"][i])
        what = "%s (texel %d)" % (t["name"][i], i)
        assert tr == bool(traced[i]), what
        if tr:
            assert np.array_equal(bits(rays["origin"][i]), bits(org)) and np.array_equal(bits(rays["direction"][i]), bits(dirs)), what
            assert rays["t_min"][i] == 0 and rays["t_max"][i] == GC.MAX_DIST
            # the image of a record with this normal: the second route's grey and confidence
            ndotl = _dot3(hn[i], [-c for c in d])
            ndotl = ndotl if not (ndotl < F(0)) else F(0)
            grey, conf = _add(F(0.5), _mul(F(0.5), ndotl)), _sub(F(1), _div(rough, t["thr"][i]))
            assert np.array_equal(bits(img[i]), bits([grey, grey, grey, conf])), what
        else:
            assert rays[i] == G.PLACEHOLDER[0], what
    return rays, traced


def test_edge_table_against_the_second_route():
    tables = GC.edge_table()
    seen = {}
    for kind, t in tables.items():
        rays, traced = check_table(t, kind)
        for name, tr in zip(t["name"], traced):
            seen.setdefault(name, set()).add(bool(tr))
    # what each edge decides
    for name in ("depth exactly 1", "the float above 1", "a NaN depth", "the float above the threshold", "a NaN roughness", "q.3 = 0",
                 "a NaN normal texel", "an infinite normal texel", "a NaN normal", "roughness in w, above"):
        assert seen[name] == {False}, name
    for name in ("the float below 1", "depth 0", "depth -0", "roughness at the threshold", "roughness -0", "on the fold, both high",
                 "on the fold, both low", "on the fold, mixed", "z exactly 0", "the corner: fx = fy = 1", "texel 0, 0", "the last pixel",
                 "identity view", "-0 matrix entries", "a zero normal", "a -0 normal", "n . d = -0", "n . d = +0, n not zero",
                 "n . d = +0, scaled", "-0 components", "facing away", "facing the viewer", "roughness in w, at"):
        assert seen[name] == {True}, name


def test_zero_normals_and_zero_dot_products():
    """A MRT_NORMAL_WORLD zero normal: dir is d and org is world.  n . d exactly zero, either sign: dir is d."""
    t = GC.edge_table()[G.NORMAL_WORLD]
    rays, traced = G.texel_rays(G.NORMAL_WORLD, t["P"], t["V"], t["thr"], GC.MAX_DIST, t["x"], t["y"], t["w"], t["h"], t["depth"], t["guide"])
    world, d, n, _ = G.texel_surface(G.NORMAL_WORLD, t["P"], t["V"], t["x"], t["y"], t["w"], t["h"], t["depth"], t["guide"])
    dot = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    names = np.asarray(t["name"])
    zero_n = np.isin(names, ["a zero normal", "a -0 normal", "n . d = -0"])
    zero_dot = zero_n | np.isin(names, ["n . d = +0, n not zero", "n . d = +0, scaled"])
    assert zero_n.sum() >= 12 and traced[zero_dot].all()
    assert (dot[zero_dot] == 0).all()
    assert np.signbit(dot[names == "n . d = -0"]).all() and not np.signbit(dot[names == "n . d = +0, n not zero"]).any()
    assert (n[names == "n . d = +0, n not zero"] != 0).any(axis=1).all()
    # by value: where a component of d is -0 (the centre column has d.x = 0) and k * n is -0, (-0) - (-0) comes back +0
    assert np.array_equal(rays["direction"][zero_dot], d[zero_dot])
    assert np.array_equal(rays["origin"][zero_n], world[zero_n])
    # facing the viewer: the mirror of d about n = -d is -d; facing away gives the same direction (k n is the same product)
    for name in ("facing the viewer", "facing away"):
        m = names == name
        np.testing.assert_allclose(rays["direction"][m], -d[m], atol=4e-7)


@pytest.mark.parametrize("kind", [G.NORMAL_OCTAHEDRAL, G.NORMAL_WORLD], ids=["octahedral", "world"])
def test_random_texels_against_the_second_route(kind):
    t = GC.random_texels(kind, 2500, seed=11 + kind)
    _, traced = check_table(t, kind)
    assert 0.3 < traced.mean() < 0.95   # both outcomes, many times


def test_frame_form_is_the_texel_form():
    """gbuffer_rays / reflection_image of a frame: pixel (x, y) is texel y * W + x; a miss's pixel is zero; lit replaces the grey."""
    w, h = 13, 7
    rng = np.random.default_rng(3)
    cam = GC.camera(w, h)
    depth = rng.uniform(0.5, 1.02, w * h).astype(F)
    guide = np.concatenate([rng.uniform(0, 1, (w * h, 2)), rng.uniform(0, 0.5, (w * h, 1)), np.zeros((w * h, 1))], axis=1).astype(F)
    g = G.GBuffer(depth, guide, cam.inv_projection, cam.inv_view, roughness_threshold=GC.THRESHOLD, max_distance=GC.MAX_DIST)
    rays, traced = G.gbuffer_rays(g, w, h)
    assert traced.any() and (~traced).any()
    i = 5 * w + 9
    one, tr = G.texel_rays(g.normal_kind, g.inv_projection, g.inv_view, g.roughness_threshold, g.max_distance, [9], [5], w, h, depth[i:i + 1], guide[i:i + 1])
    assert one[0] == rays[i] and tr[0] == traced[i]
    from messyerraytracer_amd import types as T
    hits = np.zeros(w * h, T.HIT32)
    hits["prim_id"] = np.where(traced & (rng.uniform(0, 1, w * h) < 0.7), 3, -1)
    hits["normal"] = (0.0, 1.0, 0.0)
    lit = rng.uniform(0, 2, (w * h, 4)).astype(F)
    grey, coloured = G.reflection_image(g, w, h, hits), G.reflection_image(g, w, h, hits, lit)
    miss = hits["prim_id"] == -1
    assert (grey[miss] == 0).all() and (coloured[miss] == 0).all()
    assert np.array_equal(coloured[~miss, :3], lit[~miss, :3]) and np.array_equal(coloured[:, 3], grey[:, 3])
    assert (grey[~miss, 0] >= 0.5).all() and (grey[~miss, 0] <= 1).all() and (grey[~miss, 3] >= 0).all()


# ---- the shared header, as a program of its own -------------------------------------------------------------------------------------
TEXEL = np.dtype([("kind", "<u4"), ("w", "<u4"), ("h", "<u4"), ("x", "<u4"), ("y", "<u4"), ("thr", "<f4"), ("depth", "<f4"), ("g", "<f4", 4),
                  ("P", "<f4", 16), ("V", "<f4", 16), ("prim_id", "<i4"), ("hn", "<f4", 3), ("lit", "<f4", 4)])
WANT = np.dtype([("traced", "<u4"), ("org", "<f4", 3), ("dir", "<f4", 3), ("grey", "<f4", 4), ("lit", "<f4", 4)])


def _driver_file(path):
    """the edge table and 1500 seeded texels of each kind, with a record per texel (one in four a miss), and the restatement's answers"""
    tables = GC.edge_table()
    parts = [(k, t) for k, t in tables.items()] + [(k, GC.random_texels(k, 1500, seed=101 + k)) for k in (G.NORMAL_OCTAHEDRAL, G.NORMAL_WORLD)]
    ins, wants = [], []
    rng = np.random.default_rng(17)
    for kind, t in parts:
        n = t["depth"].shape[0]
        a, w = np.zeros(n, TEXEL), np.zeros(n, WANT)
        for k in ("kind", "w", "h", "x", "y", "thr", "depth", "P", "V"):
            a[k] = t[k]
        a["g"] = t["guide"]
        a["prim_id"] = np.where(rng.uniform(0, 1, n) < 0.25, -1, rng.integers(0, 1000, n))
        a["hn"] = rng.normal(0, 1, (n, 3))
        a["lit"] = rng.uniform(0, 4, (n, 4))
        rays, traced = G.texel_rays(kind, t["P"], t["V"], t["thr"], GC.MAX_DIST, t["x"], t["y"], t["w"], t["h"], t["depth"], t["guide"])
        w["traced"], w["org"], w["dir"] = traced, rays["origin"], rays["direction"]
        w["grey"] = G.texel_image(kind, t["P"], t["V"], t["thr"], t["x"], t["y"], t["w"], t["h"], t["depth"], t["guide"], a["prim_id"], a["hn"])
        w["lit"] = G.texel_image(kind, t["P"], t["V"], t["thr"], t["x"], t["y"], t["w"], t["h"], t["depth"], t["guide"], a["prim_id"], a["hn"], a["lit"])
        ins.append(a)
        wants.append(w)
    ins, wants = np.concatenate(ins), np.concatenate(wants)
    assert TEXEL.itemsize == 204 and WANT.itemsize == 60
    with open(path, "wb") as f:
        f.write(np.uint32(ins.shape[0]).tobytes())
        f.write(ins.tobytes())
        f.write(wants.tobytes())
    return ins.shape[0]


@pytest.mark.parametrize("sanitize", [False, True])
def test_gbuffer_data_driver(tmp_path, sanitize):
    """A program of its own, with and without the sanitizers; never loaded into this process."""
    exe = mbuild.build_gbuffer_data_test(sanitize=sanitize)
    path = str(tmp_path / "gbuffer_restated.bin")
    n = _driver_file(path)
    assert n > 3000
    for args in ([], [path]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    assert ("recorded: %d texels" % n) in r.stdout, r.stdout
