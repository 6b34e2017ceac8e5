"""The textured resolve as include/mrt_hip.h states it (mrt_upload_textures; mrt_resolve_surfaces with a texture set resident) restated in
numpy on surface.py and bounce.py: TextureSampler::sample_bilinear, TriangleTangents::interpolate_tangent / interpolate_sign,
perturb_normal and all of ShadePass::extract_surface but F0 and the diffuse albedo -- float32, one operation at a time, in the order
the header states.  Test and tool plumbing (tests/test_texture_*.py, tools/bench_texture_frame.py): the device's rows, bounce pairs and
records must equal these byte for byte."""
import numpy as np

from . import bounce as B
from . import surface as S
from . import types as T

F = np.float32
NO_TEXTURE = 0xFFFFFFFF
TEXEL_RGBA8, TEXEL_RGBA32F = 0, 1
DEGENERATE = F(1e-8)
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


class TextureSet:
    """What mrt_upload_textures takes, as numpy arrays: textures, a list of [height, width, 4] arrays, uint8 (MRT_TEXEL_RGBA8) or
    float32 (MRT_TEXEL_RGBA32F); bindings [B] T.MATERIAL_TEXTURES indexed by the material id (or None); tangents12 [n, 12] float32
    {t0, t1, t2, sign0, sign1, sign2} indexed by prim_id (or None)."""

    def __init__(self, textures=(), bindings=None, tangents12=None):
        self.textures = []
        for im in textures:
            im = np.ascontiguousarray(im)
            assert im.ndim == 3 and im.shape[2] == 4 and im.dtype in (np.uint8, np.float32)
            self.textures.append(im)
        self.bindings = np.zeros(0, T.MATERIAL_TEXTURES) if bindings is None else np.ascontiguousarray(bindings, dtype=T.MATERIAL_TEXTURES)
        self.tangents12 = None if tangents12 is None else np.ascontiguousarray(tangents12, dtype=F).reshape(-1, 12)

    @property
    def n_tangent_tris(self):
        return 0 if self.tangents12 is None else self.tangents12.shape[0]


def bindings(albedo, normal, normal_scale):
    """T.MATERIAL_TEXTURES rows from three sequences (None or NO_TEXTURE: no texture)"""
    b = np.zeros(len(albedo), T.MATERIAL_TEXTURES)
    b["albedo_texture"] = [NO_TEXTURE if a is None else a for a in albedo]
    b["normal_texture"] = [NO_TEXTURE if a is None else a for a in normal]
    b["normal_scale"] = normal_scale
    return b


def texels(image, x, y):
    """Image::get_pixel as the header defines a texel: [N, 4] float32; an RGBA8 channel is (float)byte / 255.0f"""
    c = image[y, x]
    return (c.astype(F) / F(255)).astype(F) if image.dtype == np.uint8 else c.astype(F)


def lerp(a, b, t):
    """Color::lerp per channel: a + (b - a) * t"""
    return (a + ((b - a).astype(F) * t).astype(F)).astype(F)


def sample_bilinear(image, u, v):
    """TextureSampler::sample_bilinear of one image at finite u, v [N]: [N, 4] float32"""
    with np.errstate(**_QUIET):
        u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
        h, w = image.shape[:2]
        u = (u - np.floor(u)).astype(F)
        v = (v - np.floor(v)).astype(F)
        fx = ((u * F(w)).astype(F) - F(0.5)).astype(F)
        fy = ((v * F(h)).astype(F) - F(0.5)).astype(F)
        x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        sx, sy = (fx - x0.astype(F)).astype(F), (fy - y0.astype(F)).astype(F)
        x1, y1 = x0 + 1, y0 + 1
        x1, y1 = np.where(x1 >= w, x1 - w, x1), np.where(y1 >= h, y1 - h, y1)
        x0, y0 = np.where(x0 < 0, x0 + w, x0), np.where(y0 < 0, y0 + h, y0)
        assert ((x0 >= 0) & (x0 < w) & (x1 >= 0) & (x1 < w) & (y0 >= 0) & (y0 < h) & (y1 >= 0) & (y1 < h)).all()
        top = lerp(texels(image, x0, y0), texels(image, x1, y0), sx[:, None])
        bot = lerp(texels(image, x0, y1), texels(image, x1, y1), sx[:, None])
        return lerp(top, bot, sy[:, None])


def sample_textures(textures, index, u, v):
    """sample_bilinear per record: index [N] picks the record's image from the list"""
    index = np.asarray(index)
    out = np.zeros((index.shape[0], 4), F)
    for k in np.unique(index):
        m = index == k
        out[m] = sample_bilinear(textures[int(k)], np.asarray(u)[m], np.asarray(v)[m])
    return out


def _length_squared(a):
    return ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(F) + a[:, 2] * a[:, 2]).astype(F)


def _weighted(a0, a1, a2, u, v):
    w, u, v = S._weights(u, v)
    return ((a0 * w[:, None]).astype(F) + (a1 * u[:, None]).astype(F)).astype(F) + (a2 * v[:, None]).astype(F)


def interpolate_tangent(tangents12, u, v):
    """TriangleTangents::interpolate_tangent and interpolate_sign on rows [N, 12]: the tangent [N, 3] and the sign [N]"""
    with np.errstate(**_QUIET):
        t = np.asarray(tangents12, dtype=F).reshape(-1, 12)
        s = _weighted(t[:, 0:3], t[:, 3:6], t[:, 6:9], u, v).astype(F)
        l2 = _length_squared(s)
        tan = (s / np.sqrt(l2)[:, None]).astype(F)
        tan[l2 < DEGENERATE] = (1, 0, 0)
        sg = _weighted(t[:, 9:10], t[:, 10:11], t[:, 11:12], u, v).astype(F)[:, 0]
        return tan, np.where(sg >= 0, F(1), F(-1)).astype(F)


def has_tangents(tangents12):
    t = np.asarray(tangents12, dtype=F).reshape(-1, 12)
    return (t[:, 9:12] != 0).any(axis=1)


def perturb_normal(smooth, tangents12, u, v, sample, normal_scale):
    """perturb_normal past its availability checks, on [N] records: smooth [N, 3], tangent rows [N, 12] with a non-zero sign, the
    record's barycentrics, the normal map's sample [N, 4] at the record's UV, normal_scale [N]."""
    with np.errstate(**_QUIET):
        n = np.asarray(smooth, dtype=F)
        tan, bsign = interpolate_tangent(tangents12, u, v)
        k = ((n[:, 0] * tan[:, 0] + n[:, 1] * tan[:, 1]).astype(F) + n[:, 2] * tan[:, 2]).astype(F)
        tan = B.normalized((tan - (n * k[:, None]).astype(F)).astype(F))
        cross = np.stack([(n[:, 1] * tan[:, 2]).astype(F) - (n[:, 2] * tan[:, 1]).astype(F),
                          (n[:, 2] * tan[:, 0]).astype(F) - (n[:, 0] * tan[:, 2]).astype(F),
                          (n[:, 0] * tan[:, 1]).astype(F) - (n[:, 1] * tan[:, 0]).astype(F)], axis=1).astype(F)
        bit = (cross * bsign[:, None]).astype(F)
        ts = ((np.asarray(sample, dtype=F)[:, :3] * F(2)).astype(F) - F(1)).astype(F)
        scale = np.asarray(normal_scale, dtype=F)
        tsx, tsy, tsz = (ts[:, 0] * scale).astype(F), (ts[:, 1] * scale).astype(F), ts[:, 2]
        p = (((tan * tsx[:, None]).astype(F) + (bit * tsy[:, None]).astype(F)).astype(F) + (n * tsz[:, None]).astype(F)).astype(F)
        l2 = _length_squared(p)
        out = (p / np.sqrt(l2)[:, None]).astype(F)
        return np.where((l2 < DEGENERATE)[:, None], n, out).astype(F)


def resolve_textured(in_dirs, nrm, hit, prim_id, u, v, shade=None, textures=None):
    """mrt_resolve_surfaces for P records with the texture set `textures` resident (None: S.resolve).  Arguments and results as
    S.resolve: the rows [P] T.SURFACE64, the bounce pairs [P, 2] and the normals d_out_hits carries [P, 3]."""
    rows, pairs, out_n = S.resolve(in_dirs, nrm, hit, prim_id, u, v, shade)
    if textures is None or shade is None or shade.material_ids is None or shade.uvs6 is None:
        return rows, pairs, out_n                                               # no binding can apply, or no UV to sample at
    with np.errstate(**_QUIET):
        hit = np.asarray(hit, dtype=bool)
        prim = np.asarray(prim_id).astype(np.uint32)
        u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
        in_range = hit & (prim < np.uint32(shade.n_tris))
        safe = np.where(in_range, prim, 0)
        ids = np.where(in_range, shade.material_ids[safe] if shade.n_tris else 0, NO_TEXTURE).astype(np.uint32)
        bound = in_range & (ids < shade.materials.shape[0]) & (ids < textures.bindings.shape[0])
        b = textures.bindings[np.where(bound, ids, 0)] if textures.bindings.shape[0] else np.zeros(prim.shape[0], T.MATERIAL_TEXTURES)
        uv = rows["uv"]
        uv_ok = in_range & np.isfinite(uv[:, 0]) & np.isfinite(uv[:, 1])
        # the normal map
        n = out_n.copy()
        nm = bound & (b["normal_texture"] != NO_TEXTURE) & uv_ok & (prim < np.uint32(textures.n_tangent_tris))
        if nm.any():
            rows_t = textures.tangents12[np.where(nm, prim, 0)]
            nm &= has_tangents(rows_t)
        if nm.any():
            sample = sample_textures(textures.textures, b["normal_texture"][nm], uv[nm, 0], uv[nm, 1])
            n[nm] = perturb_normal(n[nm], rows_t[nm], u[nm], v[nm], sample, b["normal_scale"][nm])
            vd = B.normalized(-np.asarray(in_dirs, dtype=F)[nm])
            ndv = ((n[nm, 0] * vd[:, 0] + n[nm, 1] * vd[:, 1]).astype(F) + n[nm, 2] * vd[:, 2]).astype(F)
            rows["normal"][nm] = n[nm]
            rows["n_dot_v"][nm] = np.where(ndv < S.MIN_N_DOT_V, S.MIN_N_DOT_V, ndv)
        # the albedo texture
        am = bound & (b["albedo_texture"] != NO_TEXTURE) & uv_ok
        if am.any():
            sample = sample_textures(textures.textures, b["albedo_texture"][am], uv[am, 0], uv[am, 1])
            rows["albedo"][am] = (rows["albedo"][am] * sample[:, :3]).astype(F)
    return rows, pairs, n
