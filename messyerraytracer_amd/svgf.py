"""The SVGF pass chain of a path-traced frame as include/mrt_hip.h states it (mrt_svgf_guides, mrt_svgf_temporal, mrt_svgf_variance,
mrt_svgf_atrous, mrt_svgf_modulate, mrt_svgf_frame) restated in numpy: float32, one operation at a time, in the order the header
states, whole images at a time with a loop over the taps alone; expn_def, pow01, max_of and min_of are denoise.py's, the tone mappers
and the gamma path.py's, to_rgba8 channels.py's.  It is the standard the device is held to (tests/test_svgf_*.py,
tools/bench_svgf.py): every output word must equal these.  The ctypes wrappers of the six calls are here too.
Images are [H, W, 4] float32 (the guides of N records: [N, 4])."""
import ctypes as C

import numpy as np

from . import capi
from . import channels as Ch
from . import denoise as Dn
from . import path as P
from . import types as T

F = np.float32
SRC_RGBA, SRC_PATH_STATE = 0, 2      # MRT_ACCUM_SRC_RGBA, MRT_ACCUM_SRC_PATH_STATE
STEPS = (1, 2, 4, 8, 16)
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")
expn_def, pow01, max_of, min_of = Dn.expn_def, Dn.pow01, Dn.max_of, Dn.min_of


class SvgfParams(C.Structure):
    """mrt_svgf_params"""
    _fields_ = [("struct_size", C.c_uint32), ("has_history", C.c_uint32), ("iterations", C.c_uint32), ("tonemap_mode", C.c_uint32),
                ("color_alpha", C.c_float), ("moments_alpha", C.c_float), ("max_history", C.c_float), ("normal_threshold", C.c_float),
                ("position_threshold", C.c_float), ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_plane", C.c_float)]


def params(has_history=False, **kw):
    """mrt_svgf_params with the header's defaults"""
    p = SvgfParams()
    p.struct_size, p.has_history, p.iterations, p.tonemap_mode = C.sizeof(SvgfParams), int(bool(has_history)), 5, 0
    p.color_alpha, p.moments_alpha, p.max_history, p.normal_threshold, p.position_threshold = 0.2, 0.2, 32.0, 0.95, 0.05
    p.sigma_l, p.sigma_n, p.sigma_plane = 4.0, 128.0, 0.01
    for k, v in kw.items():
        if k not in dict(SvgfParams._fields_):
            raise TypeError(k)
        setattr(p, k, v)
    return p


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def lum(c):
    return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).astype(F)


def _img(a):
    return np.ascontiguousarray(a, dtype=F)


def guides(rays, hits, rows, radiance):
    """mrt_svgf_guides: T.RAY32, T.HIT32, T.SURFACE64 records and their radiance [N, >= 3] -> (illum, albedo, normal_depth, position)"""
    rad = _img(radiance)[:, :3]
    n = hits.shape[0]
    hit = (hits["prim_id"] != -1)[:, None]
    with np.errstate(**_QUIET):
        alb = max_of(rows["albedo"].astype(F), F(0.001))
        illum = np.zeros((n, 4), F)
        illum[:, :3] = np.where(hit, rad / alb, rad)
        albedo = np.ones((n, 4), F)
        albedo[:, :3] = np.where(hit, alb, F(1))
        nd = np.zeros((n, 4), F)
        nd[:, :3], nd[:, 3] = rows["normal"], hits["t"]
        pos = np.zeros((n, 4), F)
        pos[:, :3] = Ch.hit_position(rays["origin"], rays["direction"], hits["t"])
    return illum, albedo, np.where(hit, nd, F(0)).astype(F), np.where(hit, pos, F(0)).astype(F)


def _shift(img, tx, ty):
    """(texels at (tx, ty) clamped into the image, whether (tx, ty) lies inside)"""
    h, w = img.shape[:2]
    inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    return img[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)], inside


def reproject(cam, pos, w, h):
    """(fx, fy, whether the reprojection stands inside the window) of positions [..., 4] in the frame of capi.Camera cam"""
    o, r, u, f = (np.array(list(v), F) for v in (cam.origin, cam.right, cam.up, cam.fwd))
    with np.errstate(**_QUIET):
        e = (pos[..., :3] - o).astype(F)
        cx, cy, cz = dot3(e, r), dot3(e, u), dot3(e, f)
        wz = -cz
        uu, vv = (cx / wz) / F(cam.half_w), (cy / wz) / F(cam.half_h)
        fx = ((uu + F(1)) * F(0.5)) * F(w) - F(cam.jitter_x)
        fy = ((F(1) - vv) * F(0.5)) * F(h) - F(cam.jitter_y)
        ok = (cz < 0) & (fx >= F(-1)) & (fx < F(w)) & (fy >= F(-1)) & (fy < F(h))
    return fx.astype(F), fy.astype(F), ok


def temporal(p, illum, nd, pos, prev_cam=None, prev_illum=None, prev_moments=None, prev_nd=None, prev_pos=None):
    """mrt_svgf_temporal -> (illum with its variance, moments)"""
    illum, nd, pos = _img(illum), _img(nd), _img(pos)
    h, w = nd.shape[:2]
    with np.errstate(**_QUIET):
        l = lum(illum)
        out = illum.copy()
        out[..., 3] = 0
        mom = np.zeros((h, w, 4), F)
        mom[..., 0], mom[..., 1], mom[..., 2] = l, l * l, 1
        if p.has_history:
            pi, pm, pn, pp = _img(prev_illum), _img(prev_moments), _img(prev_nd), _img(prev_pos)
            fx, fy, ok = reproject(prev_cam, pos, w, h)
            fx, fy = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
            x0f, y0f = np.floor(fx), np.floor(fy)
            ax, ay = fx - x0f, fy - y0f
            bx, by = F(1) - ax, F(1) - ay
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            bound = F(p.position_threshold) * nd[..., 3]
            bound2 = bound * bound
            sums = np.zeros((h, w, 5), F)
            ws, n_prev, counted = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), bool)
            for k in range(4):
                i, j = k & 1, k >> 1
                tn, inside = _shift(pn, x0 + i, y0 + j)
                tp, _ = _shift(pp, x0 + i, y0 + j)
                ti, _ = _shift(pi, x0 + i, y0 + j)
                tm, _ = _shift(pm, x0 + i, y0 + j)
                d = (pos[..., :3] - tp[..., :3]).astype(F)
                take = ok & inside & (tn[..., 3] > 0) & (dot3(nd, tn) >= F(p.normal_threshold)) & (dot3(d, d) <= bound2)
                wt = (ax if i else bx) * (ay if j else by)
                vals = np.concatenate([ti[..., :3], tm[..., :2]], axis=2)
                sums = np.where(take[..., None], sums + vals * wt[..., None], sums)
                ws = np.where(take, ws + wt, ws)
                n_prev = np.where(take, np.where(counted, min_of(n_prev, tm[..., 2]), tm[..., 2]), n_prev)
                counted = counted | take
            has = ok & (ws > F(0.01))
            hist = sums / ws[..., None]
            n = min_of(n_prev + F(1), F(p.max_history))
            inv = F(1) / n
            alpha, alpha_m = max_of(F(p.color_alpha), inv), max_of(F(p.moments_alpha), inv)
            om, omm = F(1) - alpha, F(1) - alpha_m
            rgb = hist[..., :3] * om[..., None] + illum[..., :3] * alpha[..., None]
            m1 = hist[..., 3] * omm + l * alpha_m
            m2 = hist[..., 4] * omm + (l * l) * alpha_m
            var = max_of(m2 - m1 * m1, F(0))
            with_h = np.concatenate([rgb, var[..., None]], axis=2)
            mom_h = np.stack([m1, m2, n, np.zeros_like(n)], axis=2)
            out = np.where(has[..., None], with_h, out)
            mom = np.where(has[..., None], mom_h, mom)
        miss = (nd[..., 3] <= 0)[..., None]
        mom = np.where(miss, F(0), mom)
        out[..., :3] = np.where(miss, illum[..., :3], out[..., :3])
        out[..., 3] = np.where(miss[..., 0], F(0), out[..., 3])
    return out.astype(F), mom.astype(F)


def _plane_term(p, nd, pos, spos):
    d = (spos[..., :3] - pos[..., :3]).astype(F)
    return np.abs(dot3(nd, d)) / (F(p.sigma_plane) * nd[..., 3])


def variance(p, illum, moments, nd, pos):
    """mrt_svgf_variance"""
    illum, moments, nd, pos = _img(illum), _img(moments), _img(nd), _img(pos)
    h, w = nd.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(**_QUIET):
        s1, s2, ws = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                if dx == 0 and dy == 0:
                    s1, s2, ws = s1 + moments[..., 0] * F(1), s2 + moments[..., 1] * F(1), ws + F(1)
                    continue
                sn, inside = _shift(nd, xs + dx, ys + dy)
                sp, _ = _shift(pos, xs + dx, ys + dy)
                sm, _ = _shift(moments, xs + dx, ys + dy)
                dotn = dot3(nd, sn)
                take = inside & ~(sn[..., 3] <= 0) & ~(dotn <= 0)
                wt = expn_def(-_plane_term(p, nd, pos, sp)) * pow01(dotn, F(p.sigma_n))
                s1 = np.where(take, s1 + sm[..., 0] * wt, s1)
                s2 = np.where(take, s2 + sm[..., 1] * wt, s2)
                ws = np.where(take, ws + wt, ws)
        m1, m2 = s1 / ws, s2 / ws
        var = max_of(m2 - m1 * m1, F(0)) * (F(4) / moments[..., 2])
        out = illum.copy()
        out[..., 3] = np.where((nd[..., 3] <= 0) | (moments[..., 2] >= F(4)), illum[..., 3], var)
    return out.astype(F)


def b3(k):
    return F(0.375) if k == 0 else (F(0.25) if abs(k) == 1 else F(0.0625))


def atrous(p, step, illum, nd, pos):
    """mrt_svgf_atrous: one iteration at `step`"""
    illum, nd, pos = _img(illum), _img(nd), _img(pos)
    h, w = nd.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(**_QUIET):
        sv, sg = np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g = F(0.25) if (dx == 0 and dy == 0) else (F(0.125) if (dx == 0 or dy == 0) else F(0.0625))
                s, inside = _shift(illum, xs + dx, ys + dy)
                sv = np.where(inside, sv + s[..., 3] * g, sv)
                sg = np.where(inside, sg + g, sg)
        var_c = sv / sg
        denom = F(p.sigma_l) * np.sqrt(var_c) + F(1e-4)
        lc = lum(illum)
        acc, svar, ws = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                if i == 0 and j == 0:
                    wt = np.full((h, w), b3(0) * b3(0), F)
                    si, take = illum, np.ones((h, w), bool)
                else:
                    tx, ty = xs + i * step, ys + j * step
                    sn, inside = _shift(nd, tx, ty)
                    sp, _ = _shift(pos, tx, ty)
                    si, _ = _shift(illum, tx, ty)
                    dotn = dot3(nd, sn)
                    take = inside & ~(sn[..., 3] <= 0) & ~(dotn <= 0)
                    ez = _plane_term(p, nd, pos, sp)
                    el = np.abs(lc - lum(si)) / denom
                    wt = ((b3(i) * b3(j)) * expn_def(-(ez + el))) * pow01(dotn, F(p.sigma_n))
                acc = np.where(take[..., None], acc + si[..., :3] * wt[..., None], acc)
                svar = np.where(take, svar + si[..., 3] * (wt * wt), svar)
                ws = np.where(take, ws + wt, ws)
        out = np.concatenate([acc / ws[..., None], (svar / (ws * ws))[..., None]], axis=2)
        out = np.where((nd[..., 3] <= 0)[..., None], illum, out)
    return out.astype(F)


def modulate(p, illum, albedo):
    """mrt_svgf_modulate: the float image (its bytes: channels.to_rgba8)"""
    illum, albedo = _img(illum), _img(albedo)
    out = np.ones(illum.shape, F)
    with np.errstate(**_QUIET):
        c = P.tonemap((illum[..., :3] * albedo[..., :3]).astype(F), p.tonemap_mode)
        out[..., :3] = pow01(np.where(c < F(0), F(0), c).astype(F), P.GAMMA)      # path.gamma, and a NaN as it is (the C definition returns it)
    return out


def frame(p, illum, albedo, nd, pos, prev_cam=None, prev=None):
    """mrt_svgf_frame; prev = the dict of the frame before (None on the first).  Returns dict(illum, moments, nd, pos: the next
    frame's history; rgba; temporal, variance: the intermediate images)"""
    if p.has_history:
        t_illum, moments = temporal(p, illum, nd, pos, prev_cam, prev["illum"], prev["moments"], prev["nd"], prev["pos"])
    else:
        t_illum, moments = temporal(p, illum, nd, pos)
    cur = v_illum = variance(p, t_illum, moments, nd, pos)
    fed = None
    for k in range(p.iterations):
        cur = atrous(p, 1 << k, cur, nd, pos)
        if k == 0:
            fed = cur
    return dict(illum=fed, moments=moments, nd=_img(nd), pos=_img(pos), rgba=modulate(p, cur, albedo), temporal=t_illum, variance=v_illum)


# ---- the calls (ctx: a capi.Context; images: device pointers) ---------------------------------------------------------------------
_BOUND = []


def lib():
    L = capi.load()
    if not _BOUND:
        P_, V, U = C.POINTER(SvgfParams), C.c_void_p, C.c_uint32
        L.mrt_svgf_guides.argtypes = [V, V, V, V, U, V, C.c_uint64, V, V, V, V, U]
        L.mrt_svgf_temporal.argtypes = [V, P_, U, U, V, V, V, C.POINTER(capi.Camera), V, V, V, V, V, V, U]
        L.mrt_svgf_variance.argtypes = [V, P_, U, U, V, V, V, V, V, U]
        L.mrt_svgf_atrous.argtypes = [V, P_, U, U, U, V, V, V, V, U]
        L.mrt_svgf_modulate.argtypes = [V, P_, U, U, V, V, V, V, U]
        L.mrt_svgf_frame.argtypes = [V, P_, U, U, V, V, V, V, C.POINTER(capi.Camera), V, V, V, V, V, V, V, V, V, V, U]
        _BOUND.append(True)
    return L


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _cam(cam):
    return None if cam is None else C.byref(cam)


def svgf_guides(ctx, d_rays, d_hits, d_rows, source_kind, d_source, count, d_illum, d_albedo, d_nd, d_pos, flags=0):
    ctx._chk(lib().mrt_svgf_guides(ctx.h, _p(d_rays), _p(d_hits), _p(d_rows), source_kind, _p(d_source), count, _p(d_illum), _p(d_albedo),
                                   _p(d_nd), _p(d_pos), flags))


def svgf_temporal(ctx, p, w, h, d_illum, d_nd, d_pos, prev_cam, d_prev_illum, d_prev_moments, d_prev_nd, d_prev_pos, d_out_illum, d_out_moments,
                  flags=0):
    ctx._chk(lib().mrt_svgf_temporal(ctx.h, C.byref(p), w, h, _p(d_illum), _p(d_nd), _p(d_pos), _cam(prev_cam), _p(d_prev_illum),
                                     _p(d_prev_moments), _p(d_prev_nd), _p(d_prev_pos), _p(d_out_illum), _p(d_out_moments), flags))


def svgf_variance(ctx, p, w, h, d_illum, d_moments, d_nd, d_pos, d_out, flags=0):
    ctx._chk(lib().mrt_svgf_variance(ctx.h, C.byref(p), w, h, _p(d_illum), _p(d_moments), _p(d_nd), _p(d_pos), _p(d_out), flags))


def svgf_atrous(ctx, p, w, h, step, d_illum, d_nd, d_pos, d_out, flags=0):
    ctx._chk(lib().mrt_svgf_atrous(ctx.h, C.byref(p), w, h, step, _p(d_illum), _p(d_nd), _p(d_pos), _p(d_out), flags))


def svgf_modulate(ctx, p, w, h, d_illum, d_albedo, d_rgba, d_rgba8=None, flags=0):
    ctx._chk(lib().mrt_svgf_modulate(ctx.h, C.byref(p), w, h, _p(d_illum), _p(d_albedo), _p(d_rgba), _p(d_rgba8), flags))


def svgf_frame(ctx, p, w, h, d_illum, d_albedo, d_nd, d_pos, prev_cam, d_prev_illum, d_prev_moments, d_prev_nd, d_prev_pos, d_next_illum,
               d_next_moments, d_scratch_a, d_scratch_b, d_rgba, d_rgba8=None, flags=0):
    ctx._chk(lib().mrt_svgf_frame(ctx.h, C.byref(p), w, h, _p(d_illum), _p(d_albedo), _p(d_nd), _p(d_pos), _cam(prev_cam), _p(d_prev_illum),
                                  _p(d_prev_moments), _p(d_prev_nd), _p(d_prev_pos), _p(d_next_illum), _p(d_next_moments), _p(d_scratch_a),
                                  _p(d_scratch_b), _p(d_rgba), _p(d_rgba8), flags))


assert C.sizeof(SvgfParams) == 48 and T.PATH_STATE.itemsize == 32
