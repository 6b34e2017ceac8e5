"""Direct light on resolved surfaces as include/mrt_hip.h states it (mrt_light_surfaces) restated in numpy on bounce.py's `normalized`
and surface.py's rows: ShadePass::cook_torrance_multi_light and the three plain terms shade_material adds around it (analytic sky for a
miss, hemisphere ambient, emission) -- float32, one operation at a time, in the order the header states, with pow01 in float64 and
cos(spot_angle) taken from the C library's cosf.  Test and tool plumbing (tests/test_lighting_*.py, tools/bench_light_frame.py): the
device's colours must equal these byte for byte."""
import ctypes
import ctypes.util

import numpy as np

from . import bounce as B
from . import panorama as Pn
from . import types as T

F = np.float32
D = np.float64
PI = F(3.14159265358979323846)
DIFF_SCALE = F(1.0) / PI
EPS7 = F(1e-7)
EPS6 = F(1e-6)

# pow01's constants (include/mrt_hip.h states them; csrc/lighting.h holds the same literals)
LN2_HI, LN2_LO, INV_LN2 = D(6.93147180369123816490e-01), D(1.90821492927058770002e-10), D(1.44269504088896338700e+00)
SQRT2 = D(1.4142135623730951)
RND = D(6755399441055744.0)   # 1.5 * 2^52: (t + RND) - RND is t rounded to the nearest integer, ties to even
LOG_C = [D(x) for x in (2.0, 0.66666666666666663, 0.40000000000000002, 0.2857142857142857, 0.22222222222222221, 0.18181818181818182,
                        0.15384615384615385, 0.13333333333333333, 0.11764705882352941, 0.10526315789473684, 0.095238095238095233,
                        0.086956521739130432)]   # 2 / (2k + 1), k = 0 .. 11
EXP_C = [D(x) for x in (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.0083333333333333332, 0.0013888888888888889,
                        0.00019841269841269841, 2.4801587301587302e-05, 2.7557319223985893e-06, 2.7557319223985888e-07,
                        2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10)]   # 1 / k!, k = 0 .. 13
Y_ZERO, Y_INF = D(-104.0), D(89.0)   # exp(y) below 2^-150 rounds to 0 in float32; above FLT_MAX to infinity

_COSF = []


def cosf(x):
    """cosf of the C library this process runs on (what the library's host code calls): float32 in, float32 out"""
    if not _COSF:
        m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        m.cosf.restype, m.cosf.argtypes = ctypes.c_float, [ctypes.c_float]
        _COSF.append(m.cosf)
    a = np.atleast_1d(np.asarray(x, dtype=F))
    return np.array([_COSF[0](float(v)) for v in a.ravel()], dtype=F).reshape(a.shape)


def pow01(b, e):
    """b ** e for float32 b in [0, 1] and finite e >= 0, as the header defines it: selects first, otherwise exp(e * log(b)) in float64
    by + - * / alone (the exponent field is read and written as integer bits), rounded once to float32."""
    b, e = np.broadcast_arrays(np.asarray(b, dtype=F), np.asarray(e, dtype=F))
    with np.errstate(all="ignore"):
        x = np.where((b > 0) & np.isfinite(b), b, F(0.5)).astype(D)            # (lanes the selects below answer still compute)
        bits = x.view(np.int64)
        k = ((bits >> 52) & 0x7FF) - 1023
        m = ((bits & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000).view(D)
        big = m > SQRT2
        m = np.where(big, m * D(0.5), m)
        k = np.where(big, k + 1, k).astype(D)
        s = (m - D(1)) / (m + D(1))
        s2 = s * s
        q = np.full_like(s, LOG_C[11])
        for c in LOG_C[10::-1]:
            q = q * s2 + c
        lg = k * LN2_HI + (s * q + k * LN2_LO)
        y = e.astype(D) * lg
        yc = np.where((y < Y_ZERO) | (y > Y_INF) | ~np.isfinite(y), D(0), y)
        n = (yc * INV_LN2 + RND) - RND
        r = (yc - n * LN2_HI) - n * LN2_LO
        p = np.full_like(r, EXP_C[13])
        for c in EXP_C[12::-1]:
            p = p * r + c
        scale = ((n.astype(np.int64) + 1023) << 52).view(D)
        out = (p * scale).astype(F)
        out = np.where(y > Y_INF, F(np.inf), out)
        out = np.where(y < Y_ZERO, F(0), out)
        out = np.where(np.isinf(b), F(np.inf), out)
        out = np.where(b == 1, F(1), out)
        out = np.where(b == 0, F(0), out)
        out = np.where(e == 0, F(1), out)
    return out.astype(F)


def shade_lights(lights):
    """any light list as T.SHADE_LIGHT rows"""
    return np.ascontiguousarray(lights, dtype=T.SHADE_LIGHT).reshape(-1)


def shadow_lights(lights):
    """mrt_shadow_lights: the shadow half of each light as T.LIGHT rows"""
    lights = shade_lights(lights)
    out = np.zeros(lights.shape[0], T.LIGHT)
    for f in T.LIGHT.names:
        out[f] = lights[f]
    return out


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _fmax0(x):
    return np.where(x < F(0), F(0), x).astype(F)   # std::max(x, 0.0f)


def distribution_ggx(n_dot_h, roughness):
    a = roughness * roughness
    a2 = a * a
    denom = (n_dot_h * n_dot_h) * (a2 - F(1)) + F(1)
    return a2 / ((PI * denom) * denom + EPS7)


def geometry_smith_ggx(n_dot_v, n_dot_l, roughness):
    a = roughness * roughness
    a2 = a * a

    def g1(x):
        return (F(2) * x) / ((x + np.sqrt(a2 + ((F(1) - a2) * x) * x)) + EPS7)
    return g1(n_dot_v) * g1(n_dot_l)


def fresnel_schlick(cos_theta, f0):
    t = F(1) - cos_theta
    t2 = t * t
    return f0 + (F(1) - f0) * ((t2 * t2) * t)


def distance_attenuation(dist, rng, exponent):
    ratio = dist / rng
    return pow01(_fmax0(F(1) - ratio * ratio), exponent)


def spot_attenuation(L, direction, cos_outer, exponent):
    """compute_spot_attenuation(-L, direction, ...) with cos_outer = cosf(spot_angle) given: the factor and which lanes took pow01"""
    direction = np.asarray(direction, dtype=F)
    cos_angle = (L[:, 0] * direction[0] + L[:, 1] * direction[1]) + L[:, 2] * direction[2]
    inside = cos_angle > cos_outer
    t = (cos_angle - cos_outer) / (F(1) - cos_outer)
    return np.where(inside, pow01(np.where(inside, _fmax0(t), F(0)), exponent), F(0)).astype(F), inside


def light_term(rows, p, v, light, lit=None, cos_outer=None):
    """One light's term of cook_torrance_multi_light for N surfaces: rows [N] T.SURFACE64, p / v [N, 3] position and view direction
    (normalized(-d)), light one T.SHADE_LIGHT row, lit [N] the mask bytes (None: all lit).  Returns (contribution [N, 3], active [N]:
    the light was not skipped, powed [N]: the pair reached pow01, atten [N]: the attenuation where it was computed, else 1)."""
    with np.errstate(all="ignore"):
        N = rows.shape[0]
        n = rows["normal"].astype(F)
        active = np.ones(N, bool)
        powed = np.zeros(N, bool)
        atten = np.ones(N, F)
        if int(light["type"]) == T.LIGHT_DIRECTIONAL:
            L = np.tile(np.asarray(light["direction"], dtype=F), (N, 1))
        else:
            to = (np.asarray(light["position"], dtype=F)[None, :] - p).astype(F)
            dist = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2])
            active &= ~((dist < EPS6) | (dist > light["range"]))
            L = (to / dist[:, None]).astype(F)
            powed = active.copy()
            atten = np.where(active, distance_attenuation(np.where(active, dist, F(1)), light["range"], light["attenuation"]), F(1)).astype(F)
            if int(light["type"]) == T.LIGHT_SPOT:
                co = cosf(light["spot_angle"])[0] if cos_outer is None else F(cos_outer)
                spot, _ = spot_attenuation(np.where(active[:, None], L, F(0)), light["direction"], co, light["spot_angle_attenuation"])
                atten = np.where(active, atten * spot, F(1)).astype(F)
        active &= ~(atten < EPS6)
        ndl = _dot(n, L)
        active &= ~(ndl <= F(0))
        if lit is not None:
            active &= np.asarray(lit) != 0
        h = B.normalized((v + L).astype(F))
        n_dot_h, v_dot_h = _fmax0(_dot(n, h)), _fmax0(_dot(v, h))
        rough, ndv = rows["roughness"], rows["n_dot_v"]
        d_term = distribution_ggx(n_dot_h, rough)
        g_term = geometry_smith_ggx(ndv, ndl, rough)
        one_m = F(1) - rows["metallic"]
        dielectric = (F(0.04) * rows["specular"]) * F(2)
        spec_denom = (F(4) * ndv) * ndl + EPS7
        spec_scale = (d_term * g_term) / spec_denom
        out = np.zeros((N, 3), F)
        for c in range(3):
            f0 = dielectric * one_m + rows["albedo"][:, c] * rows["metallic"]
            diff = rows["albedo"][:, c] * one_m
            fr = fresnel_schlick(v_dot_h, f0)
            lc = light["color"][c] * atten
            out[:, c] = (((diff * (F(1) - fr)) * DIFF_SCALE + fr * spec_scale) * lc) * ndl
        out[~active] = 0
    return out, active, powed, atten


def view_dir(d):
    return B.normalized(-np.asarray(d, dtype=F))


def direct_light(rows, p, d, lights, mask=None, cos_outer=None):
    """cook_torrance_multi_light for N hit surfaces: d [N, 3] the incoming directions, lights T.SHADE_LIGHT rows in list order, mask
    [n_lights, N] bytes or None.  Returns (rgb [N, 3], pairs that reached pow01)."""
    lights = shade_lights(lights)
    p, v = np.asarray(p, dtype=F), view_dir(d)
    out = np.zeros((rows.shape[0], 3), F)
    n_pow = 0
    with np.errstate(all="ignore"):
        for l in range(lights.shape[0]):
            c, active, powed, _ = light_term(rows, p, v, lights[l], None if mask is None else mask[l],
                                             None if cos_outer is None else cos_outer[l])
            out = np.where(active[:, None], out + c, out).astype(F)
            n_pow += int(powed.sum())
    return out, n_pow


def sky_gradient(d, env):
    """sky_color's analytic gradient (shade_pass.h:259-274) for directions [N, 3] as given; env one T.ENVIRONMENT row"""
    d = np.asarray(d, dtype=F)
    zen, hor, gnd = (np.asarray(env[k], dtype=F) for k in ("sky_zenith", "sky_horizon", "sky_ground"))
    with np.errstate(all="ignore"):
        t = d[:, 1] * F(0.5) + F(0.5)
        up = t > F(0.5)
        s_up, s_dn = (t - F(0.5)) * F(2), t * F(2)
        hi = hor[None, :] + (zen - hor)[None, :] * s_up[:, None]
        lo = gnd[None, :] + (hor - gnd)[None, :] * s_dn[:, None]
    return np.where(up[:, None], hi, lo).astype(F)


def add_environment(rgb, r, env, panorama=None):
    """shade_material's two terms after the lights, added in place to rgb [N, 3] of the hit rows r: the ambient term (the gradient
    between ground and zenith by the normal's y, or the panorama's sample of the normal), then the emission"""
    with np.errstate(all="ignore"):
        zen, gnd, amb = (np.asarray(env[k], dtype=F) for k in ("sky_zenith", "sky_ground", "ambient"))
        blend = r["normal"][:, 1] * F(0.5) + F(0.5)
        one_m = F(1) - r["metallic"]
        sampled = None if panorama is None else Pn.sky_panorama(panorama[0], panorama[1], r["normal"])
        for c in range(3):
            a = gnd[c] + (zen[c] - gnd[c]) * blend if sampled is None else sampled[:, c]
            diff = r["albedo"][:, c] * one_m
            rgb[:, c] = rgb[:, c] + ((diff * a) * amb[c]) * F(env["ambient_energy"])
            rgb[:, c] = rgb[:, c] + r["emission"][:, c]
    return rgb


def miss_sky(miss_d, env, panorama=None):
    """what a lighting call with an environment writes for a miss: the analytic gradient, or the panorama's sample, of d as given"""
    return sky_gradient(miss_d, env) if panorama is None else Pn.sky_panorama(panorama[0], panorama[1], miss_d)


def shade_linear(rows, hit, p, d, lights, mask=None, env=None, cos_outer=None, panorama=None):
    """mrt_light_surfaces for N records: rows as mrt_resolve_surfaces wrote them, hit [N] bool, p [N, 3] positions (used for hits),
    d [N, 3] incoming directions, mask [n_lights, N] or None, env one T.ENVIRONMENT row or None, panorama (pixels [H, W, 4], energy)
    as resident (mrt_upload_panorama) or None; without env it is not read.  Returns (rgba [N, 4] float32, (pixel, light) pairs that
    reached pow01)."""
    hit = np.asarray(hit, dtype=bool)
    N = rows.shape[0]
    out = np.zeros((N, 4), F)
    idx = np.nonzero(hit)[0]
    r = rows[idx]
    rgb, n_pow = direct_light(r, np.asarray(p, dtype=F)[idx], np.asarray(d, dtype=F)[idx], lights,
                              None if mask is None else np.asarray(mask).reshape(-1, N)[:, idx], cos_outer)
    if env is not None:
        rgb = add_environment(rgb, r, env, panorama)
        out[~hit, :3] = miss_sky(np.asarray(d, dtype=F)[~hit], env, panorama)
    out[idx, :3] = rgb
    out[idx, 3] = 1
    return out, n_pow
