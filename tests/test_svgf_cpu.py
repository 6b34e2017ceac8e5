"""The SVGF pass chain without a device: the library exports the six entry points, the struct's size and layout agree and every call
refuses a null context; the restated passes (messyerraytracer_amd/svgf.py) against an independent float64 evaluation with numpy's own
exp, power and sqrt; the pure wavelet, edges between orthogonal normals, a static camera's history lengths and a disocclusion; and
the host program (csrc/host/svgf_data_test.cpp, also under AddressSanitizer and UndefinedBehaviorSanitizer as a program of its own):
every refusal in order, and the host definitions of the passes bit for bit against the restatement through a file written here."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import channels as Ch
from messyerraytracer_amd import svgf as Sv
from messyerraytracer_amd import types as T

F = np.float32
D = np.float64
U = 2.0 ** -24   # the unit roundoff of float32


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def look_basis(fwd):
    """row-major camera basis whose -z column looks along fwd, y up"""
    f = np.asarray(fwd, D) / np.linalg.norm(fwd)
    z = -f
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1).astype(F)


def camera(w, h, origin=(0.0, 0.0, 3.0), fwd=(0.0, 0.0, -1.0), fov=22.0, jitter=(0.5, 0.5)):
    return capi.ray_camera(origin, look_basis(fwd), w, h, fov, jitter=jitter)


def view_rays(cam, w, h):
    """the perspective rays of a capi.Camera as float32 (origin [3], directions [h, w, 3]); inputs of the tests, held to nothing"""
    ys, xs = np.mgrid[0:h, 0:w]
    u = (F(2) * (xs.astype(F) + F(cam.jitter_x)) * F(cam.inv_w)) - F(1)
    v = F(1) - (F(2) * (ys.astype(F) + F(cam.jitter_y)) * F(cam.inv_h))
    r, up, f = (np.array(list(a), F) for a in (cam.right, cam.up, cam.fwd))
    d = r * (u * F(cam.half_w))[..., None] + up * (v * F(cam.half_h))[..., None] - f
    return np.array(list(cam.origin), F), (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(F)


def plane_frame(cam, w, h, z=0.0, normal=(0.0, 0.0, 1.0)):
    """(normal_depth, position) of the plane through (0, 0, z) with that normal, seen by cam; a ray that misses it is a miss"""
    o, d = view_rays(cam, w, h)
    n = np.array(normal, F)
    with np.errstate(all="ignore"):
        t = (((np.array([0, 0, z], F) - o) @ n) / (d @ n)).astype(F)
    hit = np.isfinite(t) & (t > 0)
    nd, pos = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    nd[..., :3], nd[..., 3] = n, t
    pos[..., :3] = o + d * t[..., None]
    return np.where(hit[..., None], nd, F(0)).astype(F), np.where(hit[..., None], pos, F(0)).astype(F)


def images(w, h, seed, shift=0.37, x=0.0):
    """A seeded frame and the frame before it: a wall facing the camera (which stands at (x, 0, 3)) whose normals and positions are
    perturbed, illumination in [0, 1), variances in [0.01, 0.05), history lengths 1 .. 8, about 6 % misses; the previous camera stands
    `shift` pixel footprints to the left and up (a reprojection lands `shift` pixels to the right and down), and a few previous
    texels are misses, tilted or displaced.  Returns a dict of [h, w, 4] images and the two cameras."""
    rng = np.random.default_rng(seed)
    cam = camera(w, h, origin=(x, 0.0, 3.0))
    foot = 2.0 * cam.half_w * 3.0 / w
    prev_cam = camera(w, h, origin=(x - shift * foot, shift * foot, 3.0))
    out = dict(cam=cam, prev_cam=prev_cam)
    for name, c in (("", cam), ("prev_", prev_cam)):
        nd, pos = plane_frame(c, w, h)
        n = nd[..., :3] + 0.02 * rng.normal(0, 1, (h, w, 3))
        nd[..., :3] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
        pos[..., 2] += (0.002 * 3.0 * rng.uniform(-1, 1, (h, w))).astype(F)
        miss = rng.uniform(0, 1, (h, w)) < 0.06
        nd[miss], pos[miss] = 0, 0
        illum = rng.uniform(0, 1, (h, w, 4)).astype(F)
        illum[..., 3] = rng.uniform(0.01, 0.05, (h, w))
        m1 = rng.uniform(0, 1, (h, w))
        mom = np.stack([m1, m1 * m1 + rng.uniform(0, 0.05, (h, w)), rng.integers(1, 9, (h, w)), np.zeros((h, w))], axis=2).astype(F)
        out[name + "nd"], out[name + "pos"], out[name + "illum"], out[name + "moments"] = nd, pos, illum, mom
    k = max(w * h // 24, 1)
    flat = rng.integers(0, w * h, (2, k))
    out["prev_nd"].reshape(-1, 4)[flat[0], :3] = F([0.7, 0.0, 0.71414284])          # tilted: n . n_prev about 0.7
    out["prev_pos"].reshape(-1, 4)[flat[1], 2] -= F(1.0)                             # another surface, a unit behind
    out["prev_nd"][h // 2:h // 2 + 4, 0:6], out["prev_pos"][h // 2:h // 2 + 4, 0:6] = 0, 0   # a block of misses: pixels without history
    out["albedo"] = np.concatenate([rng.uniform(0.05, 1, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(F)
    return out


def test_exports_sizes_and_layouts():
    L = Sv.lib()
    for s in ("mrt_svgf_guides", "mrt_svgf_temporal", "mrt_svgf_variance", "mrt_svgf_atrous", "mrt_svgf_modulate", "mrt_svgf_frame"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert capi.STRUCT_SVGF_PARAMS == 32
    assert L.mrt_struct_size(32) == C.sizeof(Sv.SvgfParams) == 48
    assert L.mrt_struct_size(31) == 0 and L.mrt_struct_size(33) == 0
    assert [getattr(Sv.SvgfParams, n).offset for n, _ in Sv.SvgfParams._fields_] == list(range(0, 48, 4))
    p = Sv.params()
    assert (p.iterations, p.tonemap_mode, p.has_history, p.max_history, p.sigma_l, p.sigma_n) == (5, 0, 0, 32.0, 4.0, 128.0)
    assert (F(p.color_alpha), F(p.moments_alpha), F(p.normal_threshold), F(p.position_threshold), F(p.sigma_plane)) == (F(0.2), F(0.2), F(0.95), F(0.05), F(0.01))
    assert L.mrt_version() == 1
    assert L.mrt_struct_size(capi.STRUCT_GBUFFER) == 160   # the struct before it is as it was


def test_null_context_is_invalid():
    """(With a context, every bad argument is refused before any device work, in the header's order: the host program below and
    test_svgf_gpu.py.)"""
    L = Sv.lib()
    p, cam = Sv.params(), camera(4, 4)
    a = [C.c_void_p(4096 * k) for k in range(1, 16)]
    assert L.mrt_svgf_guides(None, a[0], a[1], a[2], 0, a[3], 4, a[4], a[5], a[6], a[7], 0) == capi.ERR_INVALID
    assert L.mrt_svgf_temporal(None, C.byref(p), 4, 4, a[0], a[1], a[2], C.byref(cam), a[3], a[4], a[5], a[6], a[7], a[8], 0) == capi.ERR_INVALID
    assert L.mrt_svgf_variance(None, C.byref(p), 4, 4, a[0], a[1], a[2], a[3], a[4], 0) == capi.ERR_INVALID
    assert L.mrt_svgf_atrous(None, C.byref(p), 4, 4, 1, a[0], a[1], a[2], a[3], 0) == capi.ERR_INVALID
    assert L.mrt_svgf_modulate(None, C.byref(p), 4, 4, a[0], a[1], a[2], a[3], 0) == capi.ERR_INVALID
    assert L.mrt_svgf_frame(None, C.byref(p), 4, 4, a[0], a[1], a[2], a[3], C.byref(cam), *a[4:14], 0) == capi.ERR_INVALID
    assert L.mrt_svgf_frame(None, None, 0, 0, *([None] * 4), None, *([None] * 10), 0) == capi.ERR_INVALID


# ---- an independent float64 evaluation: plain loops, numpy's own exp, power and sqrt -----------------------------------------------
def lum64(c):
    return D(F(0.2126)) * c[..., 0] + D(F(0.7152)) * c[..., 1] + D(F(0.0722)) * c[..., 2]


def _weight64(p, nd, pos, y, x, ty, tx):
    """the plane and normal factors of tap (ty, tx) for the centre (y, x), or None for a skipped tap; the caller tests the image's edge"""
    if nd[ty, tx, 3] <= 0:
        return None
    dot = nd[y, x, :3] @ nd[ty, tx, :3]
    if dot <= 0:
        return None
    ez = abs(nd[y, x, :3] @ (pos[ty, tx, :3] - pos[y, x, :3])) / (D(F(p.sigma_plane)) * nd[y, x, 3])
    return ez, np.power(dot, D(F(p.sigma_n)))


def variance64(p, illum, moments, nd, pos):
    illum, moments, nd, pos = (a.astype(D) for a in (illum, moments, nd, pos))
    h, w = nd.shape[:2]
    out = illum.copy()
    for y in range(h):
        for x in range(w):
            if nd[y, x, 3] <= 0 or moments[y, x, 2] >= 4:
                continue
            s1 = s2 = ws = 0.0
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    ty, tx = y + dy, x + dx
                    if dx == 0 and dy == 0:
                        wt = 1.0
                    elif not (0 <= tx < w and 0 <= ty < h):
                        continue
                    else:
                        f = _weight64(p, nd, pos, y, x, ty, tx)
                        if f is None:
                            continue
                        wt = np.exp(-f[0]) * f[1]
                    s1, s2, ws = s1 + moments[ty, tx, 0] * wt, s2 + moments[ty, tx, 1] * wt, ws + wt
            m1, m2 = s1 / ws, s2 / ws
            out[y, x, 3] = max(m2 - m1 * m1, 0.0) * (4.0 / moments[y, x, 2])
    return out


def atrous64(p, step, illum, nd, pos):
    illum, nd, pos = (a.astype(D) for a in (illum, nd, pos))
    h, w = nd.shape[:2]
    hk = np.array([1, 4, 6, 4, 1], D) / 16
    g3 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], D) / 16
    out = illum.copy()
    lm = lum64(illum)
    for y in range(h):
        for x in range(w):
            if nd[y, x, 3] <= 0:
                continue
            sv = sg = 0.0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= x + dx < w and 0 <= y + dy < h:
                        sv, sg = sv + illum[y + dy, x + dx, 3] * g3[dy + 1, dx + 1], sg + g3[dy + 1, dx + 1]
            denom = D(F(p.sigma_l)) * np.sqrt(sv / sg) + D(F(1e-4))
            acc, svar, ws = np.zeros(3), 0.0, 0.0
            for j in range(-2, 3):
                for i in range(-2, 3):
                    ty, tx = y + j * step, x + i * step
                    wt = hk[i + 2] * hk[j + 2]
                    if i or j:
                        if not (0 <= tx < w and 0 <= ty < h):
                            continue
                        f = _weight64(p, nd, pos, y, x, ty, tx)
                        if f is None:
                            continue
                        wt *= np.exp(-(f[0] + abs(lm[y, x] - lm[ty, tx]) / denom)) * f[1]
                    acc, svar, ws = acc + illum[ty, tx, :3] * wt, svar + illum[ty, tx, 3] * wt * wt, ws + wt
            out[y, x, :3], out[y, x, 3] = acc / ws, svar / (ws * ws)
    return out


def temporal64(p, im, w, h):
    """-> (illum, moments, the weight sum of every pixel with history, else 0)"""
    illum, nd, pos = (im[k].astype(D) for k in ("illum", "nd", "pos"))
    pi, pm, pn, pp = (im["prev_" + k].astype(D) for k in ("illum", "moments", "nd", "pos"))
    c = im["prev_cam"]
    o, r, u, f = (np.array(list(v), D) for v in (c.origin, c.right, c.up, c.fwd))
    out, mom, wsum = illum.copy(), np.zeros((h, w, 4)), np.zeros((h, w))
    out[..., 3] = 0
    for y in range(h):
        for x in range(w):
            if nd[y, x, 3] <= 0:
                continue
            l = lum64(illum[y, x])
            mom[y, x] = (l, l * l, 1, 0)
            e = pos[y, x, :3] - o
            cz = e @ f
            if not cz < 0:
                continue
            fx = ((e @ r) / -cz / c.half_w + 1) * 0.5 * w - c.jitter_x
            fy = (1 - (e @ u) / -cz / c.half_h) * 0.5 * h - c.jitter_y
            if not (-1 <= fx < w and -1 <= fy < h):
                continue
            x0, y0 = int(np.floor(fx)), int(np.floor(fy))
            ax, ay = fx - x0, fy - y0
            s, ws, n_prev = np.zeros(5), 0.0, None
            for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)):
                tx, ty = x0 + i, y0 + j
                if not (0 <= tx < w and 0 <= ty < h) or not pn[ty, tx, 3] > 0 or not nd[y, x, :3] @ pn[ty, tx, :3] >= D(F(p.normal_threshold)):
                    continue
                d = pos[y, x, :3] - pp[ty, tx, :3]
                if not d @ d <= (D(F(p.position_threshold)) * nd[y, x, 3]) ** 2:
                    continue
                wt = (ax if i else 1 - ax) * (ay if j else 1 - ay)
                s, ws = s + np.concatenate([pi[ty, tx, :3], pm[ty, tx, :2]]) * wt, ws + wt
                n_prev = pm[ty, tx, 2] if n_prev is None else min(n_prev, pm[ty, tx, 2])
            if not ws > D(F(0.01)):
                continue
            hist, n = s / ws, min(n_prev + 1, D(F(p.max_history)))
            a, am = max(D(F(p.color_alpha)), 1 / n), max(D(F(p.moments_alpha)), 1 / n)
            m1, m2 = hist[3] * (1 - am) + l * am, hist[4] * (1 - am) + l * l * am
            out[y, x, :3], out[y, x, 3] = hist[:3] * (1 - a) + illum[y, x, :3] * a, max(m2 - m1 * m1, 0.0)
            mom[y, x], wsum[y, x] = (m1, m2, n, 0), ws
    return out, mom, wsum


def test_restated_passes_against_float64():
    """Seeded 33 x 17 images (images() above: colours and moments in [0, 1), variances in [0.01, 0.05), unit normals within a few
    degrees of each other, a wall at t about 3 whose positions leave their plane by at most 0.006), default parameters, each pass of
    the restatement against float64 on the same float32 inputs.

    Tolerances, u = 2^-24, derived from the operation count before the first run and not tuned:
    a weight of the two spatial passes is a product of
      dot^128: dot of two given unit normals, 3 products and 2 sums of terms below 1: absolute error d <= 3 u; a dot below 1/2 gives a
        weight below 2^-128 that no sum notices, otherwise the relative error of dot is e <= 2 d and that of its power 128 e = 768 u.
        This term dominates.
      exp(-ez): ez = A / B, A = |n . (p_s - p_c)| by 3 differences, 3 products and 2 sums: absolute error <= 4 u S with S the sum of
        the three |n_k (p_s - p_c)_k|, here S <= 0.1 * (2.3 + 1.2) + 0.0125 < 0.363 (the view at t = 3 is 2.26 wide and 1.17 high,
        so |p_s - p_c| <= 2.3 in x and 1.2 in y, times normal components below 0.1, plus 0.0125 off the plane; all asserted below);
        B = sigma_plane * t >= 0.025 with 1 rounding, the quotient 1 more: the argument's absolute error is below
        4 u * 0.363 / 0.025 + 2 u ez, and exp turns it into a relative one of the weight; ez exp(-ez) <= 1 / e bounds what the second
        part does to a weight: 58 u + 1 u, with expn_def's own rounding 60 u.
      (a-trous alone) exp(-el): lum is 3 products and 2 sums of values below 1, absolute error 3 u, the difference of two 7 u; var_c
        is a weighted mean of 9 non-negative terms (11 u relative), its square root halves that, times sigma_l and plus 1e-4: 8 u
        relative on a denominator of at least 4 * sqrt(0.01) = 0.4: the argument moves by 7 u / 0.4 + 9 u el, which costs a weight
        18 u + 4 u = 22 u.  The sum ez + el and the one exponential: 2 u more.
      and two or three roundings for the product.
    variance pass: weight 768 + 60 + 2 = 830 u relative.  m1 and m2 are quotients of sums of at most 49 non-negative terms (a sum's
      relative error <= its worst term's + 49 u): 2 * (830 + 1 + 49) + 1 = 1761 u relative, on values below 1 and 1.05.  m2 - m1^2
      cancels: absolute error 1.05 * 1761 u + 2 * 1761 u + 2 u < 5375 u; times 4 / history_length <= 4 and two roundings: 21600 u.
    a-trous pass: weight 768 + 60 + 22 + 2 + 3 = 855 u.  rgb = a quotient of sums of at most 25 terms below 1:
      2 * (855 + 1 + 25) + 1 = 1763 u.  variance: w^2 is 2 * 855 + 1, the sum 26 more, (sum w)^2 is 2 * (855 + 25) + 1, the quotient 1:
      3499 u relative to a result that is below the largest input variance, 0.05: 175 u absolute.
    temporal pass: the reprojection.  e = p - origin 1 rounding on |e| <= 3.3; cx, cy, cz 5 more: absolute error <= 20 u each;
      cz is about -3: cx / w moves by 20 u / 3 + 0.4 * 7 u + u < 11 u, divided by half_w >= 0.19 (half_h * 33 / 17 is 0.37, half_h
      0.19): u and v move by at most 58 u + 1 u; fx = ((u + 1) * 0.5) * W - jitter: 59 u * 0.5 * 33 + 2 * 34 u < 1050 u, fy less.
      So ax, ay and their complements are off by at most 1050 u and a bilinear weight (a product of two of them, each at most 1) by
      2 * 1050 u + u < 2105 u.  The taps are the same ones: the previous camera stands 0.37 pixel to the left and up, so fx - floor(fx)
      and fy - floor(fy) stay within [0.3, 0.45] (asserted below), and no tap's test is decided near its threshold: the normals
      agree to 0.99 or, tilted, to 0.7, against 0.95; positions differ by under 0.1 or by 1, against 0.15.
      A weighted mean of values in [0, 1.05) moves by at most the sum of the four weights' errors over the weight sum, plus the
      roundings of 4 products, 3 sums and the quotient: 4 * 2105 u * 1.05 / weight_sum + 8 u.  The blend adds 3 roundings and
      alpha = max(0.2, 1 / N) one (N is exact): per pixel tol = 8841 u / weight_sum + 12 u for rgb, the same + 3 u (lum) for m1 and
      + 7 u for m2; the variance m2 - m1^2 by tol(m2) + 2 tol(m1) + 2 u.  weight_sum is float64's.
    modulate: a product, Reinhard c / (c + 1) (2 operations, all relative: 3 u in all), pow(x, 1 / 2.2) scales a relative error by
      0.46 and adds pow01's rounding: 2.4 u relative on values below 1, taken as 3 u absolute.
    guides: one quotient, 1 u relative; position 2 roundings on |o| + |d t| <= 6.2: 13 u absolute."""
    w, h = 33, 17
    im = images(w, h, 11)
    p = Sv.params(has_history=True, tonemap_mode=1)
    illum, nd, pos = im["illum"], im["nd"], im["pos"]
    # what the derivation assumes about the data
    hit = nd[..., 3] > 0
    assert hit.sum() > 0.85 * w * h and (~hit).sum() > 10
    assert (F(p.sigma_plane) * nd[..., 3][hit]).min() >= 0.025 and np.abs(nd[..., :2][hit]).max() <= 0.1
    span = np.ptp(pos[..., :3][hit], axis=0)
    assert span[0] <= 2.3 and span[1] <= 1.2 and span[2] <= 0.0125
    assert im["cam"].half_h > 0.19 and im["cam"].half_w > 0.19
    fx, fy, ok = Sv.reproject(im["prev_cam"], pos, w, h)
    assert ok[hit].mean() > 0.9
    for f_ in (fx, fy):
        assert ((f_ - np.floor(f_))[ok & hit] > 0.3).all() and ((f_ - np.floor(f_))[ok & hit] < 0.45).all()
    got_t, got_m = Sv.temporal(p, illum, nd, pos, im["prev_cam"], im["prev_illum"], im["prev_moments"], im["prev_nd"], im["prev_pos"])
    want_t, want_m, wsum = temporal64(p, im, w, h)
    has = wsum > 0
    assert has.sum() > 0.5 * w * h and (hit & ~has).sum() > 5
    np.testing.assert_array_equal(got_m[..., 2], want_m[..., 2].astype(F))            # history lengths: exact integers
    assert set(np.unique(got_m[..., 2][hit])) >= {1.0, 2.0, 5.0, 9.0}
    tol = np.where(has, 8841 * U / np.maximum(wsum, 0.01), 0) + 12 * U
    err_rgb = np.abs(got_t[..., :3].astype(D) - want_t[..., :3]).max(axis=2)
    err_m1, err_m2 = np.abs(got_m[..., 0] - want_m[..., 0]), np.abs(got_m[..., 1] - want_m[..., 1])
    err_v = np.abs(got_t[..., 3] - want_t[..., 3])
    print("temporal: rgb %.1f u, m1 %.1f u, m2 %.1f u, variance %.1f u; the smallest tolerance %.0f u" % (
        err_rgb.max() / U, err_m1.max() / U, err_m2.max() / U, err_v.max() / U, tol.min() / U))
    assert (err_rgb <= tol).all() and (err_m1 <= tol + 3 * U).all() and (err_m2 <= tol + 7 * U).all()
    assert (err_v <= 3 * tol + 15 * U).all()
    # variance
    got_v = Sv.variance(p, illum, im["moments"], nd, pos)
    want_v = variance64(p, illum, im["moments"], nd, pos)
    young = hit & (im["moments"][..., 2] < 4)
    assert young.sum() > 100 and (hit & ~young).sum() > 100
    np.testing.assert_array_equal(words(got_v[..., :3]), words(illum[..., :3]))
    np.testing.assert_array_equal(words(got_v[~young]), words(illum[~young]))
    err = np.abs(got_v[..., 3].astype(D) - want_v[..., 3]).max()
    print("variance: %.1f u of 21600 u" % (err / U))
    assert err <= 21600 * U and (got_v[young][:, 3] != illum[young][:, 3]).any()
    # a-trous, every step
    for step in Sv.STEPS:
        got_a, want_a = Sv.atrous(p, step, illum, nd, pos), atrous64(p, step, illum, nd, pos)
        e_rgb, e_var = np.abs(got_a[..., :3].astype(D) - want_a[..., :3]).max(), np.abs(got_a[..., 3].astype(D) - want_a[..., 3]).max()
        print("a-trous step %d: rgb %.1f u of 1763 u, variance %.1f u of 175 u" % (step, e_rgb / U, e_var / U))
        assert e_rgb <= 1763 * U and e_var <= 175 * U
        np.testing.assert_array_equal(words(got_a[~hit]), words(illum[~hit]))
        assert (words(got_a[hit]) != words(illum[hit])).any()
    # modulate
    got_c = Sv.modulate(p, illum, im["albedo"])
    c = illum[..., :3].astype(D) * im["albedo"][..., :3].astype(D)
    want_c = np.power(c / (c + 1), D(F(1) / F(2.2)))
    err = np.abs(got_c[..., :3] - want_c).max()
    print("modulate: %.2f u of 3 u" % (err / U))
    assert err <= 3 * U and (got_c[..., 3] == 1).all()
    # guides
    n = w * h
    rng = np.random.default_rng(3)
    rays, hits, rows = np.zeros(n, T.RAY32), np.zeros(n, T.HIT32), np.zeros(n, T.SURFACE64)
    rays["origin"], d = rng.uniform(-3, 3, (n, 3)), rng.normal(0, 1, (n, 3))
    rays["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    hits["t"], hits["prim_id"] = rng.uniform(0.1, 3, n), rng.integers(-1, 4, n)
    rows["albedo"], rows["normal"] = rng.uniform(0, 1, (n, 3)), rays["direction"]
    rows["albedo"][:8] = 0.0005
    rad = rng.uniform(0, 2, (n, 4)).astype(F)
    g_illum, g_alb, g_nd, g_pos = Sv.guides(rays, hits, rows, rad)
    hit1 = hits["prim_id"] != -1
    alb64 = np.maximum(rows["albedo"].astype(D), D(F(0.001)))
    want_i = np.where(hit1[:, None], rad[:, :3].astype(D) / alb64, rad[:, :3])
    assert (np.abs(g_illum[:, :3] - want_i) <= U * np.abs(want_i)).all() and (g_illum[:, 3] == 0).all()
    assert (g_alb[~hit1] == 1).all() and (g_alb[hit1][:, :3] == alb64[hit1].astype(F)).all() and (g_alb[:8][hit1[:8]][:, :3] == F(0.001)).all()
    want_p = rays["origin"].astype(D) + rays["direction"].astype(D) * hits["t"].astype(D)[:, None]
    assert np.abs(g_pos[hit1][:, :3] - want_p[hit1]).max() <= 13 * U and (g_pos[~hit1] == 0).all() and (g_nd[~hit1] == 0).all()
    np.testing.assert_array_equal(g_nd[hit1], np.concatenate([rows["normal"], hits["t"][:, None]], axis=1)[hit1])
    assert hit1.any() and (~hit1).any()


def flat_scene(w, h, seed, variance=0.0625):
    """a constant normal, coplanar positions (z == 0 exactly), seeded iid illumination with one variance everywhere"""
    rng = np.random.default_rng(seed)
    nd, pos = plane_frame(camera(w, h), w, h)
    assert (pos[..., 2] == 0).all() and (nd[..., 3] > 0).all()
    illum = rng.uniform(0, 1, (h, w, 4)).astype(F)
    illum[..., 3] = variance
    return illum, nd, pos


def b3_convolution64(img, step):
    """the 5 x 5 B3 convolution at `step` with taps outside the image skipped and the weights renormalised: (rgb, sum of w, sum of w^2)"""
    img = img.astype(D)
    h, w = img.shape[:2]
    hk = np.array([1, 4, 6, 4, 1], D) / 16
    acc, ws, ws2 = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    ys, xs = np.mgrid[0:h, 0:w]
    for j in range(-2, 3):
        for i in range(-2, 3):
            ty, tx = ys + j * step, xs + i * step
            inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            s = img[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1), :3]
            k = hk[i + 2] * hk[j + 2]
            acc, ws, ws2 = acc + np.where(inside[..., None], s * k, 0), ws + inside * k, ws2 + inside * k * k
    return acc / ws[..., None], ws, ws2


def test_pure_wavelet():
    """A constant normal, coplanar positions and sigma_l = 1e30: ez is exactly 0, el is below 1e-29 and its exponential exactly 1,
    pow01(1, 128) is 1: every weight is h[i] * h[j], a dyadic number.  One iteration then is the B3 convolution with skipped-border
    renormalisation: 25 products (exact but for the illumination's rounding: 1 u), a sum of 25 non-negative terms and a quotient,
    27 u relative on values below 1.  The variance channel of a constant variance v is v * sum(w^2) / sum(w)^2, in the interior
    v * (70 / 256)^2 = 0.0748 v (the same operation count: 28 u relative); and the sample variance of the filtered iid noise itself
    falls by the same factor: about 4 400 interior pixels whose filtered values correlate over the kernel's support leave that
    estimate some 300 independent samples, a relative standard deviation near sqrt(2 / 300) = 8 %: within 35 %."""
    w, h = 81, 67
    illum, nd, pos = flat_scene(w, h, 21, variance=1.0 / 12.0)
    p = Sv.params(sigma_l=1e30)
    for step in Sv.STEPS:
        got = Sv.atrous(p, step, illum, nd, pos)
        want, ws, ws2 = b3_convolution64(illum, step)
        assert np.abs(got[..., :3] - want).max() <= 27 * U
        want_v = D(illum[0, 0, 3]) * ws2 / (ws * ws)
        assert (np.abs(got[..., 3] - want_v) <= 28 * U * want_v).all()
        m = 2 * step
        inner = got[m:h - m, m:w - m]
        assert inner.size and (np.abs(inner[..., 3] / illum[0, 0, 3] - (70.0 / 256.0) ** 2) <= 30 * U).all()
        if step == 1:
            ratio = inner[..., 0].astype(D).var() / illum[m:h - m, m:w - m, 0].astype(D).var()
            print("filtered noise keeps %.4f of its variance (0.0748)" % ratio)
            assert abs(ratio / (70.0 / 256.0) ** 2 - 1) <= 0.35
        assert ws[0, 0] < 1 and ws[h // 2, w // 2] == 1


def test_edges_hold():
    """Two half-images whose normals are orthogonal (n . n = 0 is skipped): every output pixel of the variance pass and of every
    a-trous step equals what filtering its half alone gives, word for word.  The variance channel is one power of two, so that the
    3 x 3 prefilter, which looks across the edge, is exact on both sides; the luminance term stays on."""
    w, h, half = 34, 19, 17
    rng = np.random.default_rng(8)
    illum, nd, pos = flat_scene(w, h, 31)
    nd[:, half:, :3] = (1.0, 0.0, 0.0)
    pos[..., 2] = (0.001 * rng.uniform(-1, 1, (h, w))).astype(F)                       # off the plane: the plane term is on as well
    mom = np.stack([rng.uniform(0, 1, (h, w)), rng.uniform(1, 2, (h, w)), rng.integers(1, 4, (h, w)), np.zeros((h, w))], axis=2).astype(F)
    p = Sv.params(sigma_plane=10.0)                                                     # (the right half's positions are not on its plane)
    sides = (slice(0, half), slice(half, w))
    full = Sv.variance(p, illum, mom, nd, pos)
    for s in sides:
        np.testing.assert_array_equal(words(full[:, s]), words(Sv.variance(p, illum[:, s], mom[:, s], nd[:, s], pos[:, s])))
    assert (words(full[..., 3]) != words(illum[..., 3])).any()
    for step in Sv.STEPS:
        full = Sv.atrous(p, step, illum, nd, pos)
        for s in sides:
            np.testing.assert_array_equal(words(full[:, s]), words(Sv.atrous(p, step, illum[:, s], nd[:, s], pos[:, s])), err_msg=f"step {step}")
        assert (words(full[..., :3]) != words(illum[..., :3])).any()
    # with parallel normals the halves do mix
    nd[:, half:, :3] = (0.0, 0.0, 1.0)
    assert (words(Sv.atrous(p, 1, illum, nd, pos)[:, half - 2:half]) != words(Sv.atrous(p, 1, illum[:, :half], nd[:, :half], pos[:, :half])[:, half - 2:])).any()


def test_static_camera_history_lengths():
    """One quad fills the view, the camera is static and the jitter is 0.5: history_length at every pixel is exactly min(k, max_history)
    after frame k, k = 1 .. 5 (max_history 3 and 32)."""
    w, h = 33, 17
    cam = camera(w, h)
    nd, pos = plane_frame(cam, w, h)
    assert (nd[..., 3] > 0).all()
    rng = np.random.default_rng(5)
    albedo = np.ones((h, w, 4), F)
    for max_history in (3.0, 32.0):
        prev = None
        for k in range(1, 6):
            illum = rng.uniform(0, 1, (h, w, 4)).astype(F)
            illum[..., 3] = 0
            p = Sv.params(has_history=k > 1, max_history=max_history, iterations=2)
            prev = Sv.frame(p, illum, albedo, nd, pos, cam, prev)
            assert (prev["moments"][..., 2] == min(k, max_history)).all(), (k, max_history)
            assert np.isfinite(prev["rgba"]).all() and (prev["illum"][..., 3] >= 0).all()
        assert (prev["temporal"][..., 3] > 0).any()


def test_disocclusion():
    """A camera translated by one pixel footprint reprojects the interior to the neighbouring pixel, not to itself; pixels whose
    previous position lay on a different plane, farther than the threshold, restart at 1."""
    w, h = 33, 17
    prev_cam = camera(w, h)
    foot = 2.0 * prev_cam.half_w * 3.0 / w
    cam = camera(w, h, origin=(foot, 0.0, 3.0))
    nd, pos = plane_frame(cam, w, h)
    prev_nd, prev_pos = plane_frame(prev_cam, w, h)
    fx, fy, ok = Sv.reproject(prev_cam, pos, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    inner = xs < w - 1
    assert ok[inner].all() and (np.round(fx)[inner] == (xs + 1)[inner]).all() and (np.round(fy)[inner] == ys[inner]).all()
    assert (np.abs(fx - (xs + 1))[inner] < 1e-3).all() and not ok[:, w - 1].any()       # the last column left the previous view
    # a block of the previous frame showed another plane, a unit behind: farther than 0.05 * 3
    far_nd, far_pos = plane_frame(prev_cam, w, h, z=-1.0)
    block = (slice(4, 12), slice(10, 20))
    prev_nd[block], prev_pos[block] = far_nd[block], far_pos[block]
    rng = np.random.default_rng(6)
    prev_mom = np.zeros((h, w, 4), F)
    prev_mom[..., 2] = 7
    prev_illum = rng.uniform(0, 1, (h, w, 4)).astype(F)
    illum = rng.uniform(0, 1, (h, w, 4)).astype(F)
    p = Sv.params(has_history=True)
    out, mom = Sv.temporal(p, illum, nd, pos, prev_cam, prev_illum, prev_mom, prev_nd, prev_pos)
    n = mom[..., 2]
    assert (n[5:11, 10:18] == 1).all()                     # every tap in the block: x + 1 and x + 2 in 10 .. 19, y and y +- 1 in 4 .. 11
    np.testing.assert_array_equal(words(out[5:11, 10:18, :3]), words(illum[5:11, 10:18, :3]))
    assert (out[5:11, 10:18, 3] == 0).all()
    keep = np.ones((h, w), bool)
    keep[3:13, 7:21] = False
    keep[:, w - 1] = False
    assert (n[keep] == 8).all() and (n[:, w - 1] == 1).all()
    assert (words(out[keep][:, :3]) != words(illum[keep][:, :3])).any()


def _driver_file(path):
    """What the driver reads: cases on 7 x 5 (with and without history, every tone mapper), 1 x 1 and 3 x 2, each with the chain's
    results (temporal, moments, variance, five a-trous steps chained, modulate and its bytes), and guide records; little-endian"""
    rng = np.random.default_rng(5)
    cases = [(7, 5, hh, mode) for hh in (0, 1) for mode in (0, 1, 2, 3, 4)] + [(1, 1, 1, 0), (3, 2, 1, 2), (3, 2, 0, 4)]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for k, (w, h, hh, mode) in enumerate(cases):
            im = images(w, h, 100 + k, shift=0.37 if k % 2 else 1.0)
            if k % 3 == 0:
                im["illum"][0, 0, 0] = np.nan
                im["pos"][h - 1, w - 1, 1] = np.inf
                im["illum"][h // 2, w // 2, 3] = -0.25
            p = Sv.params(has_history=hh, tonemap_mode=mode, sigma_l=4.0 if k % 2 else 0.5)
            t, m = Sv.temporal(p, im["illum"], im["nd"], im["pos"], im["prev_cam"], im["prev_illum"], im["prev_moments"], im["prev_nd"], im["prev_pos"])
            v = Sv.variance(p, t, m, im["nd"], im["pos"])
            f.write(bytes(p))
            f.write(bytes(im["prev_cam"]))
            f.write(struct.pack("<II", w, h))
            for a in (im["illum"], im["albedo"], im["nd"], im["pos"], im["prev_illum"], im["prev_moments"], im["prev_nd"], im["prev_pos"], t, m, v):
                f.write(np.ascontiguousarray(a, dtype=F).tobytes())
            cur = v
            for step in Sv.STEPS:
                cur = Sv.atrous(p, step, cur, im["nd"], im["pos"])
                f.write(cur.tobytes())
            rgba = Sv.modulate(p, cur, im["albedo"])
            f.write(rgba.tobytes())
            f.write(np.ascontiguousarray(Ch.to_rgba8(rgba.reshape(-1, 4))).tobytes())
        n = 64
        rays, hits, rows = np.zeros(n, T.RAY32), np.zeros(n, T.HIT32), np.zeros(n, T.SURFACE64)
        rays["origin"], rays["direction"] = rng.uniform(-3, 3, (n, 3)), rng.normal(0, 1, (n, 3))
        hits["t"], hits["prim_id"] = rng.uniform(0, 40, n), rng.integers(-1, 3, n)
        rows["normal"], rows["albedo"] = rng.normal(0, 1, (n, 3)), rng.uniform(-0.1, 1, (n, 3))
        rows["albedo"][3, 1] = np.nan
        rad = rng.uniform(0, 4, (n, 4)).astype(F)
        out = Sv.guides(rays, hits, rows, rad)
        assert (hits["prim_id"] == -1).any() and (rows["albedo"] < 0.001).any()
        f.write(struct.pack("<I", n))
        for a in (rays, hits, rows, rad) + out:
            f.write(np.ascontiguousarray(a).tobytes())
    return len(cases), n


@pytest.mark.parametrize("sanitize", [False, True])
def test_svgf_data_driver(tmp_path, sanitize):
    """A program of its own, with and without the sanitizers; never loaded into this process."""
    exe = mbuild.build_svgf_data_test(sanitize=sanitize)
    path = str(tmp_path / "svgf_restated.bin")
    n_cases, n_guides = _driver_file(path)
    for args in ([], [path]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    assert "recorded: %d cases, %d guide records" % (n_cases, n_guides) in r.stdout
