"""The panorama sampler as include/mrt_hip.h states it (mrt_upload_panorama) restated in numpy: atan2_def and acos_def in float64 by
+ - * / and the IEEE square root alone, rounded once to float32; direction_to_equirect_uv and sample_panorama of the reference
(shade_pass.h:185-237) in float32, one operation at a time, in the reference's order.  Test and tool plumbing
(tests/test_panorama_*.py, tools/bench_panorama_frame.py): the device's colours must equal these byte for byte."""
import numpy as np

F = np.float32
D = np.float64
PI = F(3.14159265358979323846)
U_SCALE = F(0.5) / PI      # (0.5f / PI), one float constant
V_SCALE = F(1.0) / PI      # (1.0f / PI)
PI_D, PI_2, PI_4, TAN_PI_8 = D(3.141592653589793), D(1.5707963267948966), D(0.7853981633974483), D(0.41421356237309503)
ATAN_C = [D((-1.0) ** k) / D(2 * k + 1) for k in range(16)]   # (-1)^k / (2k + 1), each the correctly rounded quotient


def atan2_core(y, x):
    """core(y, x) of the header for float64 arrays: float64, not yet rounded"""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=D), np.asarray(x, dtype=D))
    with np.errstate(all="ignore"):
        yneg, xneg = np.signbit(y), np.signbit(x)
        ay, ax = np.where(yneg, -y, y), np.where(xneg, -x, x)
        steep = ay > ax
        mx, mn = np.where(steep, ay, ax), np.where(steep, ax, ay)
        zero = mx == 0
        far = mn > TAN_PI_8 * mx
        num = np.where(far, mn - mx, mn)
        den = np.where(zero, D(1), np.where(far, mn + mx, mx))
        base = np.where(far, PI_4, D(0))
        t = num / den
        t2 = t * t
        q = np.full_like(t, ATAN_C[15])
        for c in ATAN_C[14::-1]:
            q = q * t2 + c
        r = np.where(zero, D(0), base + t * q)
        r = np.where(steep, PI_2 - r, r)
        r = np.where(xneg, PI_D - r, r)
        return np.where(yneg, -r, r)


def atan2_def(y, x):
    """C99's atan2 of two finite float32 arrays as the header defines it: float64 inside, rounded once"""
    return atan2_core(np.asarray(y, dtype=F).astype(D), np.asarray(x, dtype=F).astype(D)).astype(F)


def acos_def(c):
    """acos of float32 c in [-1, 1]: core(sqrt((1 - c) * (1 + c)), c), rounded once"""
    y = np.asarray(c, dtype=F).astype(D)
    with np.errstate(all="ignore"):
        return atan2_core(np.sqrt((D(1) - y) * (D(1) + y)), y).astype(F)


def equirect_uv(d):
    """direction_to_equirect_uv for finite directions [N, 3]: (u, v) float32"""
    d = np.asarray(d, dtype=F)
    with np.errstate(all="ignore"):
        u = atan2_def(d[:, 0], d[:, 2]) * U_SCALE + F(0.5)
        c = np.where(d[:, 1] < F(-1), F(-1), np.where(d[:, 1] > F(1), F(1), d[:, 1])).astype(F)
        v = acos_def(c) * V_SCALE
    return u.astype(F), v.astype(F)


def taps(u, v, width, height):
    """sample_panorama's four taps: (x0, x1, y0, y1) int64 and (w00, w10, w01, w11) float32"""
    u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        u = u - np.floor(u)
        v = np.where(v < F(1), v, F(1)).astype(F)
        v = np.where(v > F(0), v, F(0)).astype(F)
        fx, fy = u * F(width) - F(0.5), v * F(height) - F(0.5)
        flx, fly = np.floor(fx), np.floor(fy)
        sx, sy = fx - flx, fy - fly
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        x1, y1 = x0 + 1, np.minimum(y0 + 1, height - 1)
        x1 = np.where(x1 >= width, x1 - width, x1)
        x0 = np.where(x0 < 0, x0 + width, x0)
        y0 = np.maximum(y0, 0)
        isx, isy = F(1) - sx, F(1) - sy
    return (x0, x1, y0, y1), (isx * isy, sx * isy, isx * sy, sx * sy)


def sample_panorama(pixels, u, v):
    """sample_panorama at finite (u, v): pixels [H, W, 4] float32 (alpha is not read).  Returns [N, 3] float32."""
    pixels = np.asarray(pixels, dtype=F)
    height, width = pixels.shape[:2]
    (x0, x1, y0, y1), (w00, w10, w01, w11) = taps(u, v, width, height)
    with np.errstate(all="ignore"):
        p00, p10, p01, p11 = pixels[y0, x0, :3], pixels[y0, x1, :3], pixels[y1, x0, :3], pixels[y1, x1, :3]
        out = ((p00 * w00[:, None] + p10 * w10[:, None]) + p01 * w01[:, None]) + p11 * w11[:, None]
    return out.astype(F)


def sky_panorama(pixels, energy, d):
    """sample(d) * energy of the header for directions [N, 3] as given; a direction with a non-finite component gives zeros"""
    d = np.asarray(d, dtype=F).reshape(-1, 3)
    out = np.zeros((d.shape[0], 3), F)
    ok = np.isfinite(d).all(axis=1)
    if ok.any():
        u, v = equirect_uv(d[ok])
        with np.errstate(all="ignore"):
            out[ok] = sample_panorama(pixels, u, v) * F(energy)
    return out
