"""The renderer's channels and its 8-bit image as include/mrt_hip.h states them (mrt_shade_channels, mrt_finish_color,
mrt_image_to_rgba8) restated in numpy on surface.py, texture.py and path.py: ShadePass's per-channel functions (shade_normal ..
shade_fresnel), the end of shade_material for a lit frame and RayImage::to_image -- float32, one operation at a time, in the order the
header states.  Test and tool plumbing (tests/test_channels_*.py, tools/bench_channel_frame.py): the device's planes must equal these
byte for byte."""
import numpy as np

from . import path as P
from . import surface as S
from . import texture as X

F = np.float32
COLOR, NORMAL, DEPTH, BARYCENTRIC, POSITION, PRIM_ID, HIT_MASK, ALBEDO, WIREFRAME, UV, FRESNEL, COUNT = range(12)
ALL = tuple(range(NORMAL, COUNT))
WIRE_LO, WIRE_HI, WIRE_BG = F(0.01), F(0.03), F(0.08)
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def _clamp01(x):
    return np.where(x < F(0), F(0), np.where(x > F(1), F(1), x)).astype(F)


def _frac(x):
    return (x - np.floor(x)).astype(F)


def hit_position(origins, dirs, t):
    """p = o + d * t per component: the position of a device-layout record (a host-layout record carries its own)"""
    with np.errstate(**_QUIET):
        o, d = np.asarray(origins, dtype=F), np.asarray(dirs, dtype=F)
        return (o + (d * np.asarray(t, dtype=F)[:, None]).astype(F)).astype(F)


def prim_hash(prim_id):
    """shade_prim_id's hash of a uint32: [N] uint32"""
    m, k = np.uint64(0xFFFFFFFF), np.uint64(0x45D9F3B)
    h = np.asarray(prim_id).astype(np.uint32).astype(np.uint64)
    h = (((h >> np.uint64(16)) ^ h) * k) & m
    h = (((h >> np.uint64(16)) ^ h) * k) & m
    return ((h >> np.uint64(16)) ^ h).astype(np.uint32)


def wireframe(u, v):
    """shade_wireframe's value for barycentrics [N]"""
    with np.errstate(**_QUIET):
        u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
        w = (F(1) - u) - v
        m = np.where(u < w, u, w)
        m = np.where(v < m, v, m).astype(F)
        s = _clamp01((m - WIRE_LO) / (WIRE_HI - WIRE_LO))
        e = F(1) - (s * s) * (F(3) - F(2) * s)
        return (WIRE_BG + e * (F(1) - WIRE_BG)).astype(F)


def shade_channels(in_dirs, pos, nrm, hit, t, prim_id, u, v, inv_depth_range, inv_pos_range, shade=None, textures=None, channels=ALL):
    """mrt_shade_channels for P records.  in_dirs [P, 3] the incoming directions as given, pos [P, 3] the hit positions (hit_position,
    or the host record's), nrm [P, 3] the records' normals, hit [P] bool, t, prim_id, u, v [P] the records'; shade: a S.ShadeData or
    None, textures: a X.TextureSet or None (nothing resident).  Returns {channel: [P, 4] float32} for the channels asked for."""
    out = {}
    with np.errstate(**_QUIET):
        hit = np.asarray(hit, dtype=bool)
        n_rec = hit.shape[0]
        d = np.asarray(in_dirs, dtype=F)
        prim = np.asarray(prim_id).astype(np.uint32)
        u, v, t = np.asarray(u, dtype=F), np.asarray(v, dtype=F), np.asarray(t, dtype=F)
        w = (F(1) - u) - v

        def plane(r, g, b):
            a = np.zeros((n_rec, 4), F)
            a[:, 0], a[:, 1], a[:, 2] = r, g, b
            a[~hit, :3] = 0
            a[:, 3] = 1
            return a

        if DEPTH in channels:
            x = _clamp01(F(1) - t * F(inv_depth_range))
            out[DEPTH] = plane(x, x, x)
        if BARYCENTRIC in channels:
            out[BARYCENTRIC] = plane(u, v, w)
        if POSITION in channels:
            f = _frac(np.asarray(pos, dtype=F) * F(inv_pos_range))
            out[POSITION] = plane(f[:, 0], f[:, 1], f[:, 2])
        if PRIM_ID in channels:
            h = prim_hash(prim)
            out[PRIM_ID] = plane(*((((h >> s) & 255).astype(F) / F(255)).astype(F) for s in (0, 8, 16)))
        if HIT_MASK in channels:
            out[HIT_MASK] = plane(F(1), F(1), F(1))
        if WIREFRAME in channels:
            x = wireframe(u, v)
            out[WIREFRAME] = plane(x, x, x)
        if UV in channels or FRESNEL in channels:
            rows, _, ns = S.resolve(d, nrm, hit, prim, u, v, shade)                # ns: the smooth normal
            if UV in channels:
                r = g = np.full(n_rec, F(0.5))
                if shade is not None and shade.uvs6 is not None:
                    in_range = hit & (prim < np.uint32(shade.n_tris))
                    r = np.where(in_range, _frac(rows["uv"][:, 0]), F(0.5))
                    g = np.where(in_range, _frac(rows["uv"][:, 1]), F(0.5))
                out[UV] = plane(r, g, F(0))
            if FRESNEL in channels:
                q = _clamp01((ns[:, 0] * -d[:, 0] + ns[:, 1] * -d[:, 1]) + ns[:, 2] * -d[:, 2])
                out[FRESNEL] = plane(q, q, F(0.3) + q * F(0.7))
        if NORMAL in channels or ALBEDO in channels:
            rows, _, n = X.resolve_textured(d, nrm, hit, prim, u, v, shade, textures)
            if NORMAL in channels:
                c = (n * F(0.5) + F(0.5)).astype(F)
                out[NORMAL] = plane(c[:, 0], c[:, 1], c[:, 2])
            if ALBEDO in channels:
                a = rows["albedo"]
                out[ALBEDO] = plane(a[:, 0], a[:, 1], a[:, 2])
    return out


def to_rgba8(c):
    """RayImage::to_image per component: x = c * 255 + 0.5, 0 unless 0 < x (a NaN: 0), 255 unless x < 255, truncated: uint8"""
    with np.errstate(**_QUIET):
        x = (np.asarray(c, dtype=F) * F(255) + F(0.5)).astype(F)
        x = np.where(F(0) < x, x, F(0))
        x = np.where(x < F(255), x, F(255))
        return x.astype(np.uint8)


def finish_color(lit, mode):
    """mrt_finish_color on [N, 4] float32 (what mrt_light_surfaces wrote with an environment): tone map and gamma where a != 0, the sky
    as it is elsewhere, alpha 1"""
    lit = np.asarray(lit, dtype=F)
    out = lit.copy()
    k = lit[:, 3] != 0
    out[k, :3] = P.gamma(P.tonemap(lit[k, :3], mode))
    out[:, 3] = 1
    return out
