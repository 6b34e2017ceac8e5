"""The surface of a hit record as include/mrt_hip.h states it (mrt_resolve_surfaces) restated in numpy on bounce.py's conventions:
TriangleNormals::interpolate, TriangleUV::interpolate and the material half of ShadePass::extract_surface -- float32, one operation at a
time, in the order the header states.  Test and tool plumbing (tests/test_surface_*.py, tools/bench_surface_frame.py): the device's
rows, bounce pairs and records must equal these byte for byte."""
import numpy as np

from . import bounce as B
from . import types as T

F = np.float32
MIN_N_DOT_V = F(0.001)
MIN_ROUGHNESS = F(0.04)
DEFAULT_ALBEDO, DEFAULT_METALLIC, DEFAULT_ROUGHNESS, DEFAULT_SPECULAR = F(0.75), F(0), F(0.5), F(0.5)
MISS_BOUNCE_PAIR = (F(0), F(0.5))


class ShadeData:
    """What mrt_upload_shade_data takes, as numpy arrays: materials [M] T.MATERIAL (or None), and per triangle, each optional,
    material_ids [n_tris] uint32, normals9 [n_tris, 3, 3] float32, uvs6 [n_tris, 3, 2] float32."""

    def __init__(self, n_tris=0, materials=None, material_ids=None, normals9=None, uvs6=None):
        self.n_tris = int(n_tris)
        self.materials = np.zeros(0, T.MATERIAL) if materials is None else np.ascontiguousarray(materials, dtype=T.MATERIAL)
        self.material_ids = None if material_ids is None else np.ascontiguousarray(material_ids, dtype=np.uint32)
        self.normals9 = None if normals9 is None else np.ascontiguousarray(normals9, dtype=F).reshape(-1, 3, 3)
        self.uvs6 = None if uvs6 is None else np.ascontiguousarray(uvs6, dtype=F).reshape(-1, 3, 2)
        for a in (self.material_ids, self.normals9, self.uvs6):
            assert a is None or a.shape[0] == self.n_tris


def _weights(u, v):
    u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
    return (F(1) - u) - v, u, v


def smooth_normal(n0, n1, n2, u, v):
    """TriangleNormals::interpolate on [N, 3] vertex normals: w = (1 - u) - v, (n0 * w + n1 * u) + n2 * v, normalized"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w, u, v = _weights(u, v)
        s = (np.asarray(n0, dtype=F) * w[:, None] + np.asarray(n1, dtype=F) * u[:, None]) + np.asarray(n2, dtype=F) * v[:, None]
        return B.normalized(s.astype(F))


def interpolate_uv(uv0, uv1, uv2, u, v):
    """TriangleUV::interpolate on [N, 2] vertex UVs: (uv0 * w + uv1 * u) + uv2 * v"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w, u, v = _weights(u, v)
        s = (np.asarray(uv0, dtype=F) * w[:, None] + np.asarray(uv1, dtype=F) * u[:, None]) + np.asarray(uv2, dtype=F) * v[:, None]
        return s.astype(F)


def material_surface(prim_id, shade):
    """The material half of extract_surface (shade_pass.h:535-573) for prim ids [N] (uint32): T.SURFACE64 rows with albedo, metallic,
    emission, roughness, specular and material filled, the rest zero."""
    prim = np.asarray(prim_id).astype(np.uint32)
    rows = np.zeros(prim.shape[0], T.SURFACE64)
    rows["albedo"], rows["metallic"], rows["roughness"], rows["specular"] = DEFAULT_ALBEDO, DEFAULT_METALLIC, DEFAULT_ROUGHNESS, DEFAULT_SPECULAR
    rows["material"] = T.DEFAULT_MATERIAL
    if shade is None or shade.material_ids is None:
        return rows
    in_range = prim < np.uint32(min(shade.n_tris, 0xFFFFFFFF))
    ids = np.zeros(prim.shape[0], np.uint32)
    ids[in_range] = shade.material_ids[prim[in_range]]
    k = in_range & (ids < shade.materials.shape[0])
    m = shade.materials[ids[k]]
    rows["albedo"][k], rows["metallic"][k], rows["specular"][k] = m["albedo"], m["metallic"], m["specular"]
    rows["roughness"][k] = np.where(m["roughness"] < MIN_ROUGHNESS, MIN_ROUGHNESS, m["roughness"])
    with np.errstate(over="ignore"):
        rows["emission"][k] = np.where((m["emission_energy"] > F(0))[:, None], m["emission"] * m["emission_energy"][:, None], F(0))
    rows["material"][k] = ids[k]
    return rows


def resolve(in_dirs, nrm, hit, prim_id, u, v, shade=None):
    """mrt_resolve_surfaces for P records.  in_dirs / nrm [P, 3]: incoming direction, record normal; hit [P] bool; prim_id, u, v [P]: the
    record's; shade: a ShadeData or None (nothing resident).  Returns the rows [P] T.SURFACE64, the bounce pairs [P, 2] and the
    normals d_out_hits carries [P, 3] (a miss: the record's own)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        hit = np.asarray(hit, dtype=bool)
        prim = np.asarray(prim_id).astype(np.uint32)
        nrm = np.asarray(nrm, dtype=F)
        u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
        n_tris = 0 if shade is None else shade.n_tris
        in_range = hit & (prim < np.uint32(n_tris))
        safe = np.where(in_range, prim, 0)
        n = nrm.copy()
        if shade is not None and shade.normals9 is not None and in_range.any():
            tn = shade.normals9[safe]
            n = np.where(in_range[:, None], smooth_normal(tn[:, 0], tn[:, 1], tn[:, 2], u, v), nrm).astype(F)
        vd = B.normalized(-np.asarray(in_dirs, dtype=F))
        ndv = (n[:, 0] * vd[:, 0] + n[:, 1] * vd[:, 1]) + n[:, 2] * vd[:, 2]
        rows = material_surface(np.where(hit, prim, 0xFFFFFFFF), shade)
        rows["normal"] = n
        rows["n_dot_v"] = np.where(ndv < MIN_N_DOT_V, MIN_N_DOT_V, ndv)
        if shade is not None and shade.uvs6 is not None and in_range.any():
            tu = shade.uvs6[safe]
            rows["uv"] = np.where(in_range[:, None], interpolate_uv(tu[:, 0], tu[:, 1], tu[:, 2], u, v), F(0))
        miss = np.zeros(1, T.SURFACE64)
        miss["material"] = T.DEFAULT_MATERIAL
        rows[~hit] = miss[0]
        pairs = np.stack([rows["metallic"], rows["roughness"]], axis=1).astype(F)
        pairs[~hit] = MISS_BOUNCE_PAIR
        out_n = np.where(hit[:, None], n, nrm).astype(F)
    return rows, pairs, out_n
