"""The reflection effect's image passes as include/mrt_hip.h states them (mrt_denoise_spatial, mrt_denoise_temporal,
mrt_composite_reflections, mrt_resolve_reflections, mrt_reflection_guides) restated in numpy: expn_def in float64 with lighting.py's
constants, pow01 taken from lighting.py, and the passes in float32, one operation at a time, in the order the header states.  It is
the standard the device is held to (tests/test_denoise_*.py, tools/bench_denoise.py): every output word must equal these.  The ctypes
wrappers of the five calls are here too."""
import ctypes as C

import numpy as np

from . import capi
from . import lighting as Lg
from . import types as T

F = np.float32
D = np.float64
NORMAL_OCTAHEDRAL, NORMAL_WORLD = 0, 1
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


class DenoiseParams(C.Structure):
    """mrt_denoise_params"""
    _fields_ = [("struct_size", C.c_uint32), ("normal_kind", C.c_uint32), ("has_history", C.c_uint32), ("kernel_radius", C.c_int32),
                ("depth_sigma", C.c_float), ("normal_sigma", C.c_float), ("color_sigma", C.c_float), ("blend_factor", C.c_float),
                ("depth_threshold", C.c_float), ("roughness_threshold", C.c_float), ("intensity", C.c_float), ("f0", C.c_float),
                ("inv_view", C.c_float * 16)]


def params(normal_kind=NORMAL_OCTAHEDRAL, has_history=False, inv_view=None, **kw):
    """mrt_denoise_params with the reference's defaults (rt_reflection_effect.h:43-53); inv_view: 16 floats, column-major (identity)"""
    p = DenoiseParams()
    p.struct_size, p.normal_kind, p.has_history, p.kernel_radius = C.sizeof(DenoiseParams), normal_kind, int(bool(has_history)), 2
    p.depth_sigma, p.normal_sigma, p.color_sigma, p.blend_factor = 1.0, 128.0, 4.0, 0.1
    p.depth_threshold, p.roughness_threshold, p.intensity, p.f0 = 0.1, 0.3, 1.0, 0.04
    m = np.eye(4, dtype=F).reshape(-1) if inv_view is None else np.asarray(inv_view, dtype=F).reshape(16)
    p.inv_view[:] = [float(x) for x in m]
    for k, v in kw.items():
        if k not in dict(DenoiseParams._fields_):
            raise TypeError(k)
        setattr(p, k, v)
    return p


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def expn_def(y):
    """exp(y) of float32 y <= 0 as the header defines it: float64 + - * alone, the exponent written as integer bits, rounded once"""
    y = np.asarray(y, dtype=F)
    with np.errstate(**_QUIET):
        Y = y.astype(D)
        yc = np.where((Y < Lg.Y_ZERO) | (Y > Lg.Y_INF) | np.isnan(Y), D(0), Y)
        n = (yc * Lg.INV_LN2 + Lg.RND) - Lg.RND
        r = (yc - n * Lg.LN2_HI) - n * Lg.LN2_LO
        p = np.full_like(r, Lg.EXP_C[13])
        for c in Lg.EXP_C[12::-1]:
            p = p * r + c
        scale = ((n.astype(np.int64) + 1023) << 52).view(D)
        out = (p * scale).astype(F)
        out = np.where(Y > Lg.Y_INF, F(np.inf), out)
        out = np.where(Y < Lg.Y_ZERO, F(0), out)
        out = np.where(np.isnan(y), y, out)
    return out.astype(F)


def max_of(a, b):
    return np.where(a < b, b, a).astype(F)     # a < b ? b : a


def min_of(a, b):
    return np.where(b < a, b, a).astype(F)     # b < a ? b : a


def clamp_of(x, lo, hi):
    return min_of(max_of(x, F(lo)), F(hi))


def clamp_radius(r):
    return min(max(int(r), 1), 4)


def pow01(b, e):
    """lighting.py's, and a NaN base as it is (the C definition returns it; the numpy one is only stated on the domain)"""
    b = np.asarray(b, dtype=F)
    return np.where(np.isnan(b), b, Lg.pow01(b, e)).astype(F)


def normalize3(x, y, z):
    ln = np.sqrt((x * x + y * y) + z * z)
    return x / ln, y / ln, z / ln


def decode_guide(kind, g):
    """(nx, ny, nz, roughness) of guide texels [..., 4]"""
    g = np.asarray(g, dtype=F)
    if kind == NORMAL_WORLD:
        return g[..., 0], g[..., 1], g[..., 2], g[..., 3]
    fx, fy = g[..., 0] * F(2) - F(1), g[..., 1] * F(2) - F(1)
    z = (F(1) - np.abs(fx)) - np.abs(fy)
    t = clamp_of(-z, 0, 1)
    nx = fx + np.where(fx >= 0, -t, t)
    ny = fy + np.where(fy >= 0, -t, t)
    nx, ny, nz = normalize3(nx, ny, z)
    return nx, ny, nz, g[..., 2]


def spatial_table(radius):
    """w_spatial of a clamped radius: [(2 r + 1)^2] float32, dy outer, dx inner"""
    r = int(radius)
    d = np.arange(-r, r + 1)
    d2 = (d[None, :] * d[None, :] + d[:, None] * d[:, None]).astype(F)
    with np.errstate(**_QUIET):
        return expn_def(-(d2 / (F(2) * F(r * r) + F(0.001)))).reshape(-1)


def spatial(p, refl, depth, guide):
    """mrt_denoise_spatial: refl [H, W, 4], depth [H, W], guide [H, W, 4] -> [H, W, 4]"""
    refl, depth = np.ascontiguousarray(refl, dtype=F), np.ascontiguousarray(depth, dtype=F)
    h, w = depth.shape
    r = clamp_radius(p.kernel_radius)
    table = spatial_table(r)
    ds, ns, cs = F(p.depth_sigma), F(p.normal_sigma), F(p.color_sigma)
    with np.errstate(**_QUIET):
        nx, ny, nz, _ = decode_guide(p.normal_kind, guide)
        ys, xs = np.mgrid[0:h, 0:w]
        acc = np.zeros((h, w, 4), F)
        ws = np.zeros((h, w), F)
        k = 0
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ty, tx = np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)
                s = refl[ty, tx]
                take = ~(s[..., 3] <= 0)
                dd = np.abs(depth - depth[ty, tx])
                w_depth = expn_def(-((dd * dd) * ds))
                dot = (nx * nx[ty, tx] + ny * ny[ty, tx]) + nz * nz[ty, tx]
                w_normal = pow01(max_of(dot, F(0)), ns)
                dr, dg, db = refl[..., 0] - s[..., 0], refl[..., 1] - s[..., 1], refl[..., 2] - s[..., 2]
                w_color = expn_def(-(((dr * dr + dg * dg) + db * db) * cs))
                wt = ((w_depth * w_normal) * w_color) * table[k]
                acc = np.where(take[..., None], acc + s * wt[..., None], acc)
                ws = np.where(take, ws + wt, ws)
                k += 1
        out = np.where((ws > F(0.001))[..., None], acc / ws[..., None], refl)
        out = np.where(((refl[..., 3] <= 0) | (depth >= 1))[..., None], F(0), out)
    return out.astype(F)


def temporal(p, cur, hist):
    """mrt_denoise_temporal: [..., 4] each"""
    cur = np.ascontiguousarray(cur, dtype=F)
    if not p.has_history:
        return cur.copy()
    hist = np.ascontiguousarray(hist, dtype=F)
    with np.errstate(**_QUIET):
        dd = np.abs(cur[..., 3] - hist[..., 3])
        rej = np.where(dd < F(p.depth_threshold), F(0), F(1)).astype(F)
        alpha = F(p.blend_factor) * (F(1) - rej) + rej
        om = F(1) - alpha
        out = hist * om[..., None] + cur * alpha[..., None]
        out = np.where((hist[..., 3] <= 0)[..., None], cur, out)
        out = np.where((cur[..., 3] <= 0)[..., None], hist * F(0.9), out)
    return out.astype(F)


def composite(p, refl, depth, guide, color):
    """mrt_composite_reflections: the new colour [H, W, 4]"""
    refl, depth, color = (np.ascontiguousarray(a, dtype=F) for a in (refl, depth, color))
    h, w = depth.shape
    m = np.asarray(list(p.inv_view), dtype=F).reshape(4, 4)   # m[c][r]
    with np.errstate(**_QUIET):
        nx, ny, nz, rough = decode_guide(p.normal_kind, guide)
        ys, xs = np.mgrid[0:h, 0:w]
        u, v = (xs.astype(F) + F(0.5)) / F(w), (ys.astype(F) + F(0.5)) / F(h)
        vx, vy, vz = normalize3(u * F(2) - F(1), v * F(2) - F(1), np.full((h, w), F(-1)))
        wx = (m[0][0] * vx + m[1][0] * vy) + m[2][0] * vz
        wy = (m[0][1] * vx + m[1][1] * vy) + m[2][1] * vz
        wz = (m[0][2] * vx + m[1][2] * vy) + m[2][2] * vz
        wx, wy, wz = normalize3(wx, wy, wz)
        n_dot_v = max_of((nx * -wx + ny * -wy) + nz * -wz, F(0.001))
        s = clamp_of(F(1) - n_dot_v, 0, 1)
        s2 = s * s
        s4 = s2 * s2
        s5 = s4 * s
        f0 = F(p.f0)
        fresnel = f0 + (F(1) - f0) * s5
        t = clamp_of(rough / F(p.roughness_threshold), 0, 1)
        rw = F(1) - (t * t) * (F(3) - F(2) * t)
        blend = clamp_of(((fresnel * rw) * refl[..., 3]) * F(p.intensity), 0, 1)
        om = F(1) - blend
        out = color.copy()
        rgb = color[..., :3] * om[..., None] + refl[..., :3] * blend[..., None]
        keep = (refl[..., 3] <= F(0.001)) | (depth >= 1)
        out[..., :3] = np.where(keep[..., None], color[..., :3], rgb)
    return out.astype(F)


def resolve(p, refl, depth, guide, hist, color):
    """mrt_resolve_reflections: (denoised, new history, new colour)"""
    den = spatial(p, refl, depth, guide)
    new_hist = temporal(p, den, hist)
    return den, new_hist, composite(p, new_hist, depth, guide, color)


def guides(hits, rows, inv_depth_range):
    """mrt_reflection_guides: T.HIT32 records and T.SURFACE64 rows -> (depth [N], guide [N, 4])"""
    with np.errstate(**_QUIET):
        depth = np.where(hits["prim_id"] == -1, F(1), min_of(hits["t"] * F(inv_depth_range), F(1))).astype(F)
    guide = np.concatenate([rows["normal"], rows["roughness"][:, None]], axis=1).astype(F)
    return depth, guide


# ---- the calls (ctx: a capi.Context; images: device pointers) ---------------------------------------------------------------------
_BOUND = []


def lib():
    L = capi.load()
    if not _BOUND:
        P, V, U = C.POINTER(DenoiseParams), C.c_void_p, C.c_uint32
        L.mrt_denoise_spatial.argtypes = [V, P, U, U, V, V, V, V, U]
        L.mrt_denoise_temporal.argtypes = [V, P, U, U, V, V, V, U]
        L.mrt_composite_reflections.argtypes = [V, P, U, U, V, V, V, V, U]
        L.mrt_resolve_reflections.argtypes = [V, P, U, U, V, V, V, V, V, V, U]
        L.mrt_reflection_guides.argtypes = [V, V, V, C.c_uint64, C.c_float, V, V, U]
        _BOUND.append(True)
    return L


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def denoise_spatial(ctx, p, w, h, d_reflection, d_depth, d_guide, d_out, flags=0):
    ctx._chk(lib().mrt_denoise_spatial(ctx.h, C.byref(p), w, h, _p(d_reflection), _p(d_depth), _p(d_guide), _p(d_out), flags))


def denoise_temporal(ctx, p, w, h, d_current, d_history, d_out, flags=0):
    ctx._chk(lib().mrt_denoise_temporal(ctx.h, C.byref(p), w, h, _p(d_current), _p(d_history), _p(d_out), flags))


def composite_reflections(ctx, p, w, h, d_reflection, d_depth, d_guide, d_color, flags=0):
    ctx._chk(lib().mrt_composite_reflections(ctx.h, C.byref(p), w, h, _p(d_reflection), _p(d_depth), _p(d_guide), _p(d_color), flags))


def resolve_reflections(ctx, p, w, h, d_reflection, d_depth, d_guide, d_history, d_color, d_denoised=None, flags=0):
    ctx._chk(lib().mrt_resolve_reflections(ctx.h, C.byref(p), w, h, _p(d_reflection), _p(d_depth), _p(d_guide), _p(d_history), _p(d_color),
                                           _p(d_denoised), flags))


def reflection_guides(ctx, d_hits, d_rows, count, inv_depth_range, d_depth, d_guide, flags=0):
    ctx._chk(lib().mrt_reflection_guides(ctx.h, _p(d_hits), _p(d_rows), count, inv_depth_range, _p(d_depth), _p(d_guide), flags))


assert C.sizeof(DenoiseParams) == 112 and T.HIT32.itemsize == 32
