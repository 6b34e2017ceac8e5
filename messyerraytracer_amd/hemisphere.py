"""The cosine-weighted hemisphere ray of include/mrt_hip.h restated in numpy: the reference's PCG32 and the jump constants that reach
a draw without stepping through the ones before it, the sincos pair, Duff's orthonormal basis, the direction and the ray -- float32,
one operation at a time, in the order the header states.  Test and tool plumbing (tests/test_hemisphere_*.py,
tools/bench_hemisphere_frame.py): the device's rays must equal these byte for byte."""
import numpy as np

from . import types as T

F = np.float32
U = np.uint32
MUL, INC = 747796405, 2891336453
M32 = 0xFFFFFFFF
T_MIN, BIAS = F(1e-4), F(1e-3)
HALF_PI = F(1.5707964e+00)
SIN_COEF = (F(-2.5052108e-08), F(2.7557319e-06), F(-1.984127e-04), F(8.333334e-03), F(-1.6666667e-01))   # x^11 .. x^3 (Taylor)
COS_COEF = (F(-2.755732e-07), F(2.4801588e-05), F(-1.3888889e-03), F(4.1666668e-02), F(-5.0e-01))        # x^10 .. x^2


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & np.uint64(M32)


def pcg_state0(seed):
    """PCG32::seed: the state after seeding (uint64 arrays holding 32-bit values, as everything here)"""
    return _u32((np.uint64(INC) + _u32(seed)) * np.uint64(MUL) + np.uint64(INC))


def pcg_step(state):
    return _u32(_u32(state) * np.uint64(MUL) + np.uint64(INC))


def pcg_output(state):
    """what PCG32::next returns from the state it finds"""
    s = _u32(state)
    word = _u32(((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737))
    return ((word >> np.uint64(22)) ^ word).astype(U)


def to_float(out):
    """PCG32::next_float's scaling: float(uint32) (round to nearest even) * 2^-32 -- 1.0 for outputs from 0xFFFFFF80 up"""
    return np.asarray(out, dtype=U).astype(F) * F(2.0 ** -32)


def jump(k):
    """(A, C) with: state before draw k = A * state0 + C (mod 2^32); draw 0 is the first after seeding."""
    a, c = 1, 0
    for _ in range(int(k)):
        a, c = (a * MUL) & M32, (c * MUL + INC) & M32
    return a, c


def draw(seed, k):
    """draw number k of the stream seeded with `seed`, through the jump constants: uint32"""
    a, c = jump(k)
    return pcg_output(_u32(np.uint64(a) * pcg_state0(seed) + np.uint64(c)))


def draws(seed, n):
    """the first n draws of each seed by stepping, [..., n] uint32"""
    s = pcg_state0(seed)
    out = []
    for _ in range(n):
        out.append(pcg_output(s))
        s = pcg_step(s)
    return np.stack(out, axis=-1)


def sincos_2pi(u):
    """(cos, sin) of 2 pi u for float32 u in [0, 1]: quadrant reduction (exact) and two fixed polynomials"""
    u = np.asarray(u, dtype=F)
    a = u * F(4)
    k = np.rint(a)
    f = a - k
    x = f * HALF_PI
    x2 = x * x
    s = np.full_like(x, SIN_COEF[0])
    for c in SIN_COEF[1:]:
        s = s * x2 + c
    s = x + (x * x2) * s
    co = np.full_like(x, COS_COEF[0])
    for c in COS_COEF[1:]:
        co = co * x2 + c
    co = F(1) + x2 * co
    q = k.astype(np.int32) & 3
    cs = np.where(q == 0, co, np.where(q == 1, -s, np.where(q == 2, -co, s)))
    sn = np.where(q == 0, s, np.where(q == 1, co, np.where(q == 2, -s, -co)))
    return cs.astype(F), sn.astype(F)


def onb(n):
    """construct_onb (Duff et al.) of unit normals [N, 3]: tangent, bitangent"""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sign = np.copysign(F(1), nz)
    a = F(-1) / (sign + nz)
    b = (nx * ny) * a
    t = np.stack([F(1) + ((sign * nx) * nx) * a, sign * b, (-sign) * nx], axis=1)
    bt = np.stack([b, sign + (ny * ny) * a, -ny], axis=1)
    return t.astype(F), bt.astype(F)


def direction(n, u1, u2):
    """cosine_hemisphere_sample's direction around the normals n [N, 3] for the draws u1, u2 (float32 [N])"""
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.asarray(n, dtype=F)
        r = np.sqrt(u1)
        z = np.sqrt(np.maximum(F(0), F(1) - u1))
        cs, sn = sincos_2pi(u2)
        x, y = r * cs, r * sn
        t, bt = onb(n)
        v = (t * x[:, None] + bt * y[:, None]) + n * z[:, None]
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        d = v / np.sqrt(l2)[:, None]
        d[l2 == 0] = 0
    return d.astype(F)


def sample_direction(seed, n, first_draw=0, sample=0):
    """the direction for the stream of `seed` [N] around n [N, 3]: draws first_draw + 2 * sample and the next one"""
    u1 = to_float(draw(seed, first_draw + 2 * sample))
    u2 = to_float(draw(seed, first_draw + 2 * sample + 1))
    return direction(n, u1, u2), u1, u2


PLACEHOLDER = np.zeros(1, dtype=T.RAY32)  # the reference's Ray(0, (0, 1, 0), 0, 0) for entries without a ray
PLACEHOLDER["direction"] = (0.0, 1.0, 0.0)


def hemisphere_rays(in_dirs, pos, nrm, hit, pixel_index, n_samples, frame, first_draw, t_max, select=None):
    """The rays of a hemisphere cast, [n_samples * pixels] mrt_ray32 in entry order (sample-major), the mask of entries with a ray and
    the mask of pixels whose normal was turned.  in_dirs / pos / nrm [P, 3]: incoming direction, hit position, record normal; hit [P]
    bool; pixel_index [P]."""
    with np.errstate(over="ignore", invalid="ignore"):
        P = in_dirs.shape[0]
        d = np.asarray(in_dirs, dtype=F)
        n = np.asarray(nrm, dtype=F).copy()
        flip = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] > F(0)
        n[flip] = -n[flip]
        ok = np.asarray(hit, dtype=bool).copy()
        if select is not None:
            ok &= np.asarray(select) != 0
        seed = _u32(_u32(np.asarray(pixel_index, dtype=np.uint64) * np.uint64(1009)) + np.uint64((frame * 6529 + 7) & M32))
        rays = np.zeros(n_samples * P, dtype=T.RAY32)
        traced = np.zeros(n_samples * P, dtype=bool)
        org = np.asarray(pos, dtype=F) + n * BIAS
        nn = np.where(ok[:, None], n, np.array([0, 0, 1], dtype=F))  # (entries without a record: any unit normal, the result unused)
        for s in range(n_samples):
            dirs, _, _ = sample_direction(seed, nn, first_draw, s)
            above = (nn[:, 0] * dirs[:, 0] + nn[:, 1] * dirs[:, 1]) + nn[:, 2] * dirs[:, 2] > F(0)
            r = rays[s * P:(s + 1) * P]
            r["origin"], r["direction"], r["t_min"], r["t_max"] = org, dirs, T_MIN, F(t_max)
            tr = ok & above
            r[~tr] = PLACEHOLDER[0]
            traced[s * P:(s + 1) * P] = tr
    return rays, traced, flip & ok
