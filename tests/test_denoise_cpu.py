"""The reflection effect's image passes without a device: the library exports the five entry points, the struct's size and layout
agree and every call refuses a null argument; expn_def (messyerraytracer_amd/denoise.py) against numpy's exp on a dense sweep; the
restated passes against an independent float64 evaluation of the shader formulas; and the host program
(csrc/host/denoise_data_test.cpp, also under AddressSanitizer and UndefinedBehaviorSanitizer as a program of its own): every refusal
in order, the w_spatial tables, the radius clamp, and the host definitions of expn_def and of the four passes bit for bit against the
restatement through a file written here."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import denoise as Dn
from messyerraytracer_amd import types as T

F = np.float32
D = np.float64
U = 2.0 ** -24   # the unit roundoff of float32

_SWEEP = []


def sweep():
    """every -j * 2^-12 for j in 0 .. 2^19 (down to -128), plus 2^20 seeded arguments in [-110, 0]: (arguments, expn_def of them)"""
    if not _SWEEP:
        y = np.concatenate([-(np.arange(2 ** 19 + 1, dtype=D) * 2.0 ** -12), np.random.default_rng(2024).uniform(-110.0, 0.0, 2 ** 20)]).astype(F)
        _SWEEP.append((y, Dn.expn_def(y)))
    return _SWEEP[0]


def images(w, h, seed, kind):
    """seeded images with colours and depths in [0, 1): some alphas 0, a few sky depths, unit WORLD normals or any octahedral pair"""
    rng = np.random.default_rng(seed)
    refl = rng.uniform(0, 1, (h, w, 4)).astype(F)
    refl[..., 3] = np.where(rng.uniform(0, 1, (h, w)) < 0.2, 0, refl[..., 3])
    depth = rng.uniform(0, 1, (h, w)).astype(F)
    depth.reshape(-1)[rng.integers(0, w * h, max(w * h // 16, 1))] = 1.0
    guide = rng.uniform(0, 1, (h, w, 4)).astype(F)
    if kind == Dn.NORMAL_WORLD:
        n = rng.normal(0, 1, (h, w, 3)) * 0.2 + np.array([0.0, 1.0, 0.3])
        guide[..., :3] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    else:
        guide[..., :2] = (0.5 + 0.12 * rng.normal(0, 1, (h, w, 2))).clip(0, 1).astype(F)   # a narrow cone: the normal weight matters
    hist = rng.uniform(0, 1, (h, w, 4)).astype(F)
    hist[..., 3] = np.where(rng.uniform(0, 1, (h, w)) < 0.2, 0, refl[..., 3] + rng.choice(F([0, 0.01, 0.3]), (h, w)))
    color = rng.uniform(0, 1, (h, w, 4)).astype(F)
    return refl, depth, guide, hist, color


def rotation():
    a, b = 0.6, -0.35
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx
    m[:3, 3] = (1.0, 2.0, 3.0)
    return m.T.astype(F).reshape(-1)   # column-major


def test_exports_sizes_and_layouts():
    L = Dn.lib()
    for s in ("mrt_denoise_spatial", "mrt_denoise_temporal", "mrt_composite_reflections", "mrt_resolve_reflections", "mrt_reflection_guides"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert capi.STRUCT_DENOISE_PARAMS == 28
    assert L.mrt_struct_size(28) == C.sizeof(Dn.DenoiseParams) == 112
    assert L.mrt_struct_size(27) == 0 and L.mrt_struct_size(29) == 0
    assert [getattr(Dn.DenoiseParams, n).offset for n, _ in Dn.DenoiseParams._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48]
    p = Dn.params()
    assert (p.kernel_radius, p.depth_sigma, p.normal_sigma, p.color_sigma) == (2, 1.0, 128.0, 4.0)
    assert (F(p.blend_factor), F(p.depth_threshold), F(p.roughness_threshold), p.intensity, F(p.f0)) == (F(0.1), F(0.1), F(0.3), 1.0, F(0.04))
    assert L.mrt_version() == 1
    assert L.mrt_struct_size(capi.STRUCT_ACCUM_STATE) == C.sizeof(capi.AccumState)   # the struct before it is as it was


def test_null_arguments_are_invalid():
    """(With a context, every bad argument is refused before any device work, in the order the driver checks: test_denoise_gpu.py.)"""
    L = Dn.lib()
    p = Dn.params()
    a, b, c, d, e, f = (C.c_void_p(4096 * k) for k in range(1, 7))
    assert L.mrt_denoise_spatial(None, C.byref(p), 4, 4, a, b, c, d, 0) == capi.ERR_INVALID
    assert L.mrt_denoise_temporal(None, C.byref(p), 4, 4, a, b, c, 0) == capi.ERR_INVALID
    assert L.mrt_composite_reflections(None, C.byref(p), 4, 4, a, b, c, d, 0) == capi.ERR_INVALID
    assert L.mrt_resolve_reflections(None, C.byref(p), 4, 4, a, b, c, d, e, f, 0) == capi.ERR_INVALID
    assert L.mrt_reflection_guides(None, a, b, 4, 1.0, c, d, 0) == capi.ERR_INVALID
    assert L.mrt_denoise_spatial(None, None, 0, 0, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.mrt_resolve_reflections(None, None, 0, 0, None, None, None, None, None, None, 0) == capi.ERR_INVALID


def test_expn_def_is_within_one_ulp_of_exp():
    """fp64 Horner to degree 13 on |r| <= ln2 / 2 is exact to about 1e-16 relative, far below half a float32 ulp (6e-8), so the one
    rounding to float32 can differ from the correctly rounded exp only at a near-tie: at most 1 ulp, and rarely.  Measured on this
    sweep: N_DIFFER = 0 arguments of 1,572,865 differ at all."""
    N_DIFFER = 0
    y, got = sweep()
    with np.errstate(under="ignore"):
        want = np.exp(y.astype(D)).astype(F)
    assert (got[y < F(-104)] == 0).all() and (got[y >= F(-103.9)] > 0).all()
    keep = y >= F(-104)     # below: flushed to 0 by definition (exp is under 2^-150 there, which rounds to 0 as well)
    assert (want[~keep] == 0).all()
    ulps = np.abs(got[keep].view(np.int32).astype(np.int64) - want[keep].view(np.int32).astype(np.int64))
    print("expn_def: %d of %d arguments differ from the rounded exp, at most %d ulp" % ((ulps != 0).sum(), y.size, ulps.max()))
    assert ulps.max() <= 1
    assert (ulps != 0).sum() == N_DIFFER
    assert got[0] == 1 and Dn.expn_def(F(-0.0)) == 1 and np.isnan(Dn.expn_def(F(np.nan))) and Dn.expn_def(F(90)) == np.inf
    assert Dn.expn_def(F(1)) == F(np.e)


def test_pow01_just_above_one():
    """The dot of two normalised vectors can be a few ulps above 1: pow01 has no select for it and computes b^e like any other."""
    b = F(1) + F(2.0 ** -23) * np.arange(1, 9, dtype=F)
    got = Dn.pow01(b, F(128))
    want = np.power(b.astype(D), 128.0).astype(F)
    assert (got > 1).all() and np.abs(got.view(np.int32) - want.view(np.int32)).max() <= 1
    assert got[1] == F(1.0000305)   # b = 1 + 2^-22, the header's example
    assert np.isnan(Dn.pow01(F(np.nan), F(128)))


# ---- an independent float64 evaluation of the shader formulas, numpy's own exp and power -----------------------------------------
def _decode64(kind, g):
    g = g.astype(D)
    if kind == Dn.NORMAL_WORLD:
        return g[..., :3], g[..., 3]
    f = g[..., :2] * 2 - 1
    n = np.concatenate([f, (1 - np.abs(f[..., 0]) - np.abs(f[..., 1]))[..., None]], axis=2)
    t = np.clip(-n[..., 2], 0, 1)
    n[..., 0] += np.where(n[..., 0] >= 0, -t, t)
    n[..., 1] += np.where(n[..., 1] >= 0, -t, t)
    return n / np.linalg.norm(n, axis=2, keepdims=True), g[..., 2]


def spatial64(p, refl, depth, guide):
    refl, depth = refl.astype(D), depth.astype(D)
    h, w = depth.shape
    n, _ = _decode64(p.normal_kind, guide)
    r = min(max(p.kernel_radius, 1), 4)
    out = np.zeros((h, w, 4))
    for y in range(h):
        for x in range(w):
            if refl[y, x, 3] <= 0 or depth[y, x] >= 1:
                continue
            total, wsum = np.zeros(4), 0.0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    ty, tx = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
                    s = refl[ty, tx]
                    if s[3] <= 0:
                        continue
                    wt = np.exp(-(depth[y, x] - depth[ty, tx]) ** 2 * p.depth_sigma) * np.power(max(n[y, x] @ n[ty, tx], 0.0), p.normal_sigma)
                    cd = refl[y, x, :3] - s[:3]
                    wt *= np.exp(-(cd @ cd) * p.color_sigma) * np.exp(-(dx * dx + dy * dy) / (2.0 * r * r + D(F(0.001))))
                    total += s * wt
                    wsum += wt
            out[y, x] = total / wsum if wsum > 0.001 else refl[y, x]
    return out


def temporal64(p, cur, hist):
    cur, hist = cur.astype(D), hist.astype(D)
    rej = (np.abs(cur[..., 3] - hist[..., 3]) >= D(F(p.depth_threshold))).astype(D)
    alpha = (p.blend_factor * (1 - rej) + rej)[..., None]
    out = hist * (1 - alpha) + cur * alpha
    out = np.where((hist[..., 3] <= 0)[..., None], cur, out)
    return np.where((cur[..., 3] <= 0)[..., None], hist * D(F(0.9)), out)


def composite64(p, refl, depth, guide, color):
    refl, color = refl.astype(D), color.astype(D)
    h, w = depth.shape
    n, rough = _decode64(p.normal_kind, guide)
    m = np.array(list(p.inv_view), D).reshape(4, 4).T[:3, :3]
    ys, xs = np.mgrid[0:h, 0:w]
    v = np.stack([(xs + 0.5) / w * 2 - 1, (ys + 0.5) / h * 2 - 1, -np.ones((h, w))], axis=2)
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    v = v @ m.T
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    ndv = np.maximum(-(n * v).sum(axis=2), D(F(0.001)))
    fres = p.f0 + (1 - p.f0) * np.clip(1 - ndv, 0, 1) ** 5
    t = np.clip(rough / p.roughness_threshold, 0, 1)
    blend = np.clip(fres * (1 - t * t * (3 - 2 * t)) * refl[..., 3] * p.intensity, 0, 1)[..., None]
    out = color.copy()
    out[..., :3] = color[..., :3] * (1 - blend) + refl[..., :3] * blend
    return np.where(((refl[..., 3] <= D(F(0.001))) | (depth >= 1))[..., None], color, out)


@pytest.mark.parametrize("kind", [Dn.NORMAL_WORLD, Dn.NORMAL_OCTAHEDRAL])
def test_restated_passes_against_float64(kind):
    """33 x 17 images, colours and depths in [0, 1), default sigmas, r = 2, each pass against float64 on the same float32 inputs.

    Tolerances, u = 2^-24, derived before the first run and not tuned:
    spatial.  A weight is a product of four factors.  w_depth, w_color, w_spatial are exps of arguments made by 4, 7 and 4 float32
      operations with |argument| <= 1, 12 (three squared differences below 1, times sigma 4) and 1: the argument's absolute error,
      at most 4 u, 84 u and 4 u, is the factor's relative error; with expn_def's own rounding of each, under 100 u for the three
      together.  w_normal = dot^128: a relative error e of dot
      becomes 128 e.  dot < 1/2 gives a weight below 2^-128, which no sum notices; for dot >= 1/2, e <= 2 d, d the absolute error of
      dot.  WORLD normals are given: d <= 3 u (three products, two sums, |terms| <= 1), so 128 * 6 u = 768 u.  Octahedral normals
      are decoded by 5 operations and a normalisation per component, an absolute error below 6 u each on vectors of length 1, so
      d <= 2 * sqrt(3) * 6 u + 3 u < 24 u and 128 * 48 u = 6144 u.  Three more roundings for the product of the four.  sum and
      weight_sum are sums of at most 25 non-negative terms (relative error of the sum <= the largest of its terms' + 25 u), and their
      quotient doubles it:  2 * (768 + 100 + 3 + 25 + 1) u = 1794 u for WORLD, 2 * (6144 + 129) u = 12546 u for OCTAHEDRAL,
      relative to each component (all terms are in [0, 1), so the same bound holds absolutely).
    temporal.  Four operations on values in [0, 1.3): 4 * 1.3 u, taken as 6 u absolute.
    composite.  The view vector: 2 normalisations and a 3x3 product, below 16 u absolute per component; NdotV 16 u * sqrt(3) + 3 u
      + the normal's own 6 u * sqrt(3) < 48 u; (1 - NdotV)^5 at most 5 * 48 u = 240 u, times (1 - f0) < 1; smoothstep 6 operations
      with slope <= 1.5 on roughness / threshold (2 u): 12 u; the product of four factors below 1: 256 u in all for blend; the mix of
      two values in [0, 1) moves by at most that plus 3 u: 260 u absolute."""
    w, h = 33, 17
    refl, depth, guide, hist, color = images(w, h, 7 + kind, kind)
    p = Dn.params(normal_kind=kind, has_history=True, inv_view=rotation())
    den = Dn.spatial(p, refl, depth, guide)
    want = spatial64(p, refl, depth, guide)
    tol_spatial = (1794 if kind == Dn.NORMAL_WORLD else 12546) * U
    err_s = np.abs(den.astype(D) - want).max()
    assert (den[(refl[..., 3] <= 0) | (depth >= 1)] == 0).all() and (den != 0).any()
    new_hist = Dn.temporal(p, den, hist)
    err_t = np.abs(new_hist.astype(D) - temporal64(p, den, hist)).max()
    out = Dn.composite(p, new_hist, depth, guide, color)
    err_c = np.abs(out.astype(D) - composite64(p, new_hist, depth, guide, color)).max()
    print("kind %d: spatial %.3g (%.1f u), temporal %.3g (%.1f u), composite %.3g (%.1f u)" % (kind, err_s, err_s / U, err_t, err_t / U, err_c, err_c / U))
    assert err_s <= tol_spatial
    assert err_t <= 6 * U
    assert err_c <= 260 * U
    assert (out[..., 3] == color[..., 3]).all() and (out != color).any()
    # the fused form is the three in sequence
    d2, h2, c2 = Dn.resolve(p, refl, depth, guide, hist, color)
    assert (d2.view(np.uint32) == den.view(np.uint32)).all() and (h2.view(np.uint32) == new_hist.view(np.uint32)).all()
    assert (c2.view(np.uint32) == out.view(np.uint32)).all()
    # without history the temporal pass is the identity
    p.has_history = 0
    assert (Dn.temporal(p, den, hist).view(np.uint32) == den.view(np.uint32)).all()


def _driver_file(path):
    """What the driver reads: the expn_def sweep, the tables of r = 1 .. 4, cases of both kinds on 7 x 5 (and a 1 x 1 and a 3 x 2 at
    r = 4) with the three results, and a handful of guide records; little-endian"""
    y, e = sweep()
    rng = np.random.default_rng(5)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", y.size))
        f.write(y.tobytes())
        f.write(e.tobytes())
        for r in (1, 2, 3, 4):
            f.write(Dn.spatial_table(r).tobytes())
        cases = [(7, 5, kind, radius, hh) for kind in (0, 1) for radius in (1, 2, 4) for hh in (0, 1)] + [(1, 1, 0, 2, 1), (3, 2, 1, 9, 1)]
        f.write(struct.pack("<I", len(cases)))
        for k, (w, h, kind, radius, hh) in enumerate(cases):
            refl, depth, guide, hist, color = images(w, h, 100 + k, kind)
            if k % 3 == 0:
                refl[0, 0, 0] = np.nan
                guide[h - 1, w - 1] = 0          # a zero WORLD normal / the octahedral corner
            p = Dn.params(normal_kind=kind, has_history=hh, inv_view=rotation() if k % 2 else None, kernel_radius=radius)
            den, nh, nc = Dn.resolve(p, refl, depth, guide, hist, color)
            f.write(bytes(p))
            f.write(struct.pack("<II", w, h))
            for a in (refl, depth, guide, hist, color, den, nh, nc):
                f.write(np.ascontiguousarray(a, dtype=F).tobytes())
        n = 64
        hits, rows = np.zeros(n, T.HIT32), np.zeros(n, T.SURFACE64)
        hits["t"], hits["prim_id"] = rng.uniform(0, 40, n), rng.integers(-1, 3, n)
        rows["normal"], rows["roughness"] = rng.normal(0, 1, (n, 3)), rng.uniform(0, 1, n)
        d, g = Dn.guides(hits, rows, F(0.05))
        assert (d == 1).any() and (d < 1).any() and (hits["prim_id"] == -1).any()
        f.write(struct.pack("<I", n))
        for a in (hits, rows, np.array([0.05], F), d, g):
            f.write(np.ascontiguousarray(a).tobytes())
    return len(cases), n


@pytest.mark.parametrize("sanitize", [False, True])
def test_denoise_data_driver(tmp_path, sanitize):
    """A program of its own, with and without the sanitizers; never loaded into this process."""
    exe = mbuild.build_denoise_data_test(sanitize=sanitize)
    path = str(tmp_path / "denoise_restated.bin")
    n_cases, n_guides = _driver_file(path)
    for args in ([], [path]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    assert "recorded: %d exp arguments, %d cases, %d guide records" % (sweep()[0].size, n_cases, n_guides) in r.stdout
