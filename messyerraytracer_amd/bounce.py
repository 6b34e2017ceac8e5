"""The bounce ray of include/mrt_hip.h (mrt_cast_bounce) restated in numpy on top of hemisphere.py: the specular probability, the GGX
half vector, the lobe choice and the direction of either lobe, the ray and the lobe byte -- float32, one operation at a time, in the
order the header states.  Test and tool plumbing (tests/test_bounce_*.py, tools/bench_bounce_frame.py): the device's rays and lobe
bytes must equal these byte for byte."""
import numpy as np

from . import hemisphere as H
from . import types as T

F = np.float32
LOBE_NONE, LOBE_DIFFUSE, LOBE_SPECULAR = 0, 1, 2
EPS = F(1e-7)
MIN_ROUGHNESS = F(0.04)


def jump(k):
    """(A, C) with: state before draw k = A * state0 + C (mod 2^32), by squaring the step as the library's host code does: any k"""
    A, C, a, c, k = 1, 0, H.MUL, H.INC, int(k) & H.M32
    while k:
        if k & 1:
            A, C = (a * A) & H.M32, (a * C + c) & H.M32
        c, a, k = (a * c + c) & H.M32, (a * a) & H.M32, k >> 1
    return A, C


def draw(seed, k):
    """draw number k of the stream seeded with `seed`, through the jump constants: uint32"""
    a, c = jump(k)
    return H.pcg_output(H._u32(np.uint64(a) * H.pcg_state0(seed) + np.uint64(c)))


def clamp_surface(metallic, roughness):
    """m, ro: fminf(fmaxf(x, lower), 1) -- a NaN takes the lower bound, as fmaxf returns its other argument"""
    m = np.fmin(np.fmax(np.asarray(metallic, dtype=F), F(0)), F(1))
    ro = np.fmin(np.fmax(np.asarray(roughness, dtype=F), MIN_ROUGHNESS), F(1))
    return m.astype(F), ro.astype(F)


def spec_prob(m, ro):
    """sample_bounce's lobe-selection probability from the clamped pair"""
    sp = m + ((F(1) - m) * (F(1) - ro)) * F(0.5)
    return np.fmax(np.fmin(sp, F(0.95)), F(0.05)).astype(F)


def normalized(v):
    """Vector3::normalized on [N, 3]: (x*x + y*y) + z*z, sqrt, three divisions; 0 where the sum is 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        d = v / np.sqrt(l2)[:, None]
        d[l2 == 0] = 0
    return d.astype(F)


def ggx_half(n, ro, u1, u2):
    """ggx_sample_half around the normals n [N, 3] for the draws u1, u2: the half vector, cos_theta, sin_theta"""
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.asarray(n, dtype=F)
        a = ro * ro
        a2 = a * a
        c = np.sqrt((F(1) - u1) / ((F(1) + (a2 - F(1)) * u1) + EPS))
        s = np.sqrt(np.maximum(F(0), F(1) - c * c))
        cs, sn = H.sincos_2pi(u2)
        lx, ly = s * cs, s * sn
        t, bt = H.onb(n)
        h = normalized((t * lx[:, None] + bt * ly[:, None]) + n * c[:, None])
    return h, c.astype(F), s.astype(F)


def bounce_direction(n, d, m, ro, u0, u1, u2):
    """The direction of sample_bounce around the (faced) normals n [N, 3] for incoming directions d [N, 3], the clamped pair and the
    three draws: direction [N, 3], specular [N] bool, the specular probability, the half vector (rows of diffuse entries unused)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = np.asarray(n, dtype=F)
        sp = spec_prob(m, ro)
        specular = u0 < sp
        diffuse_dir = H.direction(n, u1, u2)
        h, _, _ = ggx_half(n, ro, u1, u2)
        v = normalized(-np.asarray(d, dtype=F))
        vh = np.maximum((v[:, 0] * h[:, 0] + v[:, 1] * h[:, 1]) + v[:, 2] * h[:, 2], F(0))
        spec_dir = normalized(h * (F(2) * vh)[:, None] - v)
    return np.where(specular[:, None], spec_dir, diffuse_dir).astype(F), specular, sp, h


def bounce_rays(in_dirs, pos, nrm, hit, pixel_index, frame, first_draw, t_max, metallic, roughness, select=None):
    """The rays of a bounce cast, [P] mrt_ray32 in record order, the mask of entries with a ray and the lobe bytes.  in_dirs / pos / nrm
    [P, 3]: incoming direction, hit position, record normal; hit [P] bool; pixel_index [P]; metallic, roughness: scalars or [P]."""
    with np.errstate(over="ignore", invalid="ignore"):
        P = in_dirs.shape[0]
        d = np.asarray(in_dirs, dtype=F)
        n = np.asarray(nrm, dtype=F).copy()
        flip = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] > F(0)
        n[flip] = -n[flip]
        ok = np.asarray(hit, dtype=bool).copy()
        if select is not None:
            ok &= np.asarray(select) != 0
        seed = H._u32(H._u32(np.asarray(pixel_index, dtype=np.uint64) * np.uint64(1009)) + np.uint64((frame * 6529 + 7) & H.M32))
        u0, u1, u2 = (H.to_float(draw(seed, first_draw + k)) for k in range(3))
        m, ro = clamp_surface(np.broadcast_to(np.asarray(metallic, dtype=F), (P,)), np.broadcast_to(np.asarray(roughness, dtype=F), (P,)))
        nn = np.where(ok[:, None], n, np.array([0, 0, 1], dtype=F))  # (entries without a record: any unit normal, the result unused)
        dd = np.where(ok[:, None], d, np.array([0, 0, -1], dtype=F))
        dirs, specular, _, _ = bounce_direction(nn, dd, m, ro, u0, u1, u2)
        above = ~((nn[:, 0] * dirs[:, 0] + nn[:, 1] * dirs[:, 1]) + nn[:, 2] * dirs[:, 2] <= F(0))  # (the kernel's test: "no ray if <= 0")
        traced = ok & above
        rays = np.zeros(P, dtype=T.RAY32)
        rays["origin"], rays["direction"] = np.asarray(pos, dtype=F) + n * H.BIAS, dirs
        rays["t_min"], rays["t_max"] = H.T_MIN, F(t_max)
        rays[~traced] = H.PLACEHOLDER[0]
        lobe = np.where(traced, np.where(specular, LOBE_SPECULAR, LOBE_DIFFUSE), LOBE_NONE).astype(np.uint8)
    return rays, traced, lobe
