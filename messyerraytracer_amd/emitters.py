"""Emissive triangles as light sources, as include/mrt_hip.h states them (mrt_build_emitters, mrt_cast_emitter_shadows,
mrt_light_emitter_surfaces, mrt_path_step_emitters), restated in numpy from what the other restatements hold: the stream and its jump
(hemisphere.py, bounce.py), the surface terms and the step (path.py), the resolve's material rule (surface.py).  Its own rules are the
table (integer weights, so that no sum depends on its order), the selection with an exact pmf, the point on the triangle, the three
refusals and the diffuse term -- float32, one operation at a time, in the order the header states.  Test and tool plumbing
(tests/test_emitters_*.py, tools/bench_emitter_nee.py): the device's table, words, bytes and floats must equal these word for word."""
import numpy as np

from . import bounce as B
from . import hemisphere as H
from . import path as P
from . import types as T

F = np.float32
INV_PI = F(0.31830988618)
LUMA = (F(0.2126), F(0.7152), F(0.0722))
TWO31 = F(2147483648.0)
EPS6 = F(1e-6)
SELF_SHADOW = F(0.999)


def cross(a, b):
    """e1 x e2 per component, as the header writes it"""
    with np.errstate(all="ignore"):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                         a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F)


def triangle_weights(tris, shade):
    """Per triangle of T.TRI64 rows: Le [N, 3], area [N], w [N] (0 where the triangle is no emitter) and the material id [N].  shade: a
    surface.ShadeData or None."""
    tris = np.ascontiguousarray(tris, dtype=T.TRI64)
    n = tris.shape[0]
    le = np.zeros((n, 3), F)
    material = np.full(n, T.DEFAULT_MATERIAL, np.uint32)
    with np.errstate(all="ignore"):
        if shade is not None and shade.material_ids is not None and shade.materials.shape[0]:
            in_range = tris["id"] < np.uint32(min(shade.n_tris, 0xFFFFFFFF))
            ids = np.zeros(n, np.uint32)
            ids[in_range] = shade.material_ids[tris["id"][in_range]]
            k = in_range & (ids < shade.materials.shape[0])
            m = shade.materials[ids[k]]
            le[k] = np.where((m["emission_energy"] > F(0))[:, None], m["emission"] * m["emission_energy"][:, None], F(0))
            material[k] = ids[k]
        c = cross(tris["edge1"].astype(F), tris["edge2"].astype(F))
        area = F(0.5) * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        w = area * ((LUMA[0] * le[:, 0] + LUMA[1] * le[:, 1]) + LUMA[2] * le[:, 2])
        w = np.where((w > F(0)) & np.isfinite(w), w, F(0)).astype(F)
    return le, area.astype(F), w, material


def ceil_log2(n):
    return max(int(n) - 1, 0).bit_length()


def integer_weights(w):
    """q [n] uint32 and the inclusive cdf [n] uint32 of float32 weights w > 0: w_max, Q = 2^(31 - ceil_log2(n)), q0 = max(1,
    uint32((w / w_max) * Q)), T0 = sum q0, q = (q0 << 31) // T0."""
    w = np.asarray(w, dtype=F)
    n = w.shape[0]
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    Q = F(2.0 ** (31 - ceil_log2(n)))
    q0 = np.maximum(((w / w.max()) * Q).astype(np.int64), 1)
    t0 = int(q0.sum())
    q = ((q0.astype(np.uint64) << np.uint64(31)) // np.uint64(t0)).astype(np.uint64)
    return q.astype(np.uint32), np.cumsum(q, dtype=np.uint64).astype(np.uint32)


def build_table(tris, shade):
    """mrt_build_emitters: (rows [n] T.EMITTER64, cdf [n] uint32) for T.TRI64 triangles and a surface.ShadeData (None: 0 emitters).
    More than T.MAX_EMITTERS emitters: ValueError (the call returns MRT_ERR_UNSUPPORTED)."""
    tris = np.ascontiguousarray(tris, dtype=T.TRI64)
    le, area, w, material = triangle_weights(tris, shade)
    on = np.flatnonzero(w > F(0))
    if on.size > T.MAX_EMITTERS:
        raise ValueError("more than MAX_EMITTERS emitters")
    rows = np.zeros(on.size, T.EMITTER64)
    t = tris[on]
    rows["v0"], rows["edge1"], rows["edge2"], rows["prim_id"] = t["v0"], t["edge1"], t["edge2"], t["id"]
    rows["area"], rows["radiance"], rows["material"] = area[on], le[on], material[on]
    rows["q"], cdf = integer_weights(w[on])
    return rows, cdf


def select_emitters(cdf, words):
    """k [N] uint32 for selecting words [N]: target = word >> 1; T.EMITTER_NONE where target >= total (or the table is empty), else the
    first entry with cdf[k] > target."""
    words = np.asarray(words, dtype=np.uint32)
    out = np.full(words.shape[0], T.EMITTER_NONE, np.uint32)
    if len(cdf):
        target = words >> np.uint32(1)
        ok = target < cdf[-1]
        out[ok] = np.searchsorted(cdf, target[ok], side="right").astype(np.uint32)
    return out


def triangle_point(u1, u2):
    """(a, b) of the point v0 + e1 * a + e2 * b for the two floats: su = sqrt(u1), a = su * (1 - u2), b = su * u2"""
    su = np.sqrt(np.asarray(u1, dtype=F))
    u2 = np.asarray(u2, dtype=F)
    return (su * (F(1) - u2)).astype(F), (su * u2).astype(F)


def emitter_samples(in_dirs, pos, nrm, hit, pixel_index, frame, draw, rows, cdf, select=None, emitter=None):
    """What mrt_cast_emitter_shadows derives for N records, as a dict: emitter [N] uint32 (d_out_emitter), traced [N] bool (a ray is
    cast), rays [N] mrt_ray32 (the placeholder where none is), and of the sampled point dir [N, 3], dist2, ndl, cy, plus the faced normal
    n.  in_dirs / pos / nrm [N, 3]: incoming direction, hit position, record normal; hit [N] bool; pixel_index [N]; rows, cdf: the
    table.  emitter: instead of selecting, the words to take (mrt_light_emitter_surfaces reads the cast's)."""
    with np.errstate(all="ignore"):
        N = in_dirs.shape[0]
        d = np.asarray(in_dirs, dtype=F)
        n = np.asarray(nrm, dtype=F).copy()
        flip = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] > F(0)
        n[flip] = -n[flip]
        hit = np.asarray(hit, dtype=bool)
        seed = P.stream_seed(pixel_index, frame)
        if emitter is None:
            on = hit.copy() if select is None else hit & (np.asarray(select) != 0)
            k = np.where(on, select_emitters(cdf, B.draw(seed, draw)), np.uint32(T.EMITTER_NONE)).astype(np.uint32)
        else:
            k = np.where(hit, np.asarray(emitter, dtype=np.uint32), np.uint32(T.EMITTER_NONE)).astype(np.uint32)
        has = k < np.uint32(len(cdf))
        r = rows[np.where(has, k, 0)] if len(cdf) else np.zeros(N, T.EMITTER64)
        a, b = triangle_point(H.to_float(B.draw(seed, draw + 1)), H.to_float(B.draw(seed, draw + 2)))
        y = (r["v0"] + r["edge1"] * a[:, None]) + r["edge2"] * b[:, None]
        org = np.asarray(pos, dtype=F) + n * H.BIAS
        to = (y - org).astype(F)
        dist2 = (to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2]
        dist = np.sqrt(dist2)
        dirs = (to / dist[:, None]).astype(F)
        ndl = (n[:, 0] * dirs[:, 0] + n[:, 1] * dirs[:, 1]) + n[:, 2] * dirs[:, 2]
        ng = B.normalized(cross(r["edge1"], r["edge2"]))
        cy = np.abs((ng[:, 0] * dirs[:, 0] + ng[:, 1] * dirs[:, 1]) + ng[:, 2] * dirs[:, 2])
        traced = has & ~(dist < EPS6) & ~(ndl <= F(0)) & ~(cy < EPS6)
        rays = np.zeros(N, T.RAY32)
        rays["origin"], rays["direction"], rays["t_min"], rays["t_max"] = org, dirs, F(0), dist * SELF_SHADOW
        rays[~traced] = H.PLACEHOLDER[0]
    return dict(emitter=k, traced=traced, rays=rays, dir=dirs, dist2=dist2.astype(F), ndl=ndl.astype(F), cy=cy.astype(F), n=n, row=r)


def emitter_terms(surface_rows, sample, mask=None):
    """The term of N hit records [N, 3]: 0 where no ray was cast or the mask byte is 0."""
    with np.errstate(all="ignore"):
        _, diff = P.surface_terms(surface_rows)
        r = sample["row"]
        geom = (sample["ndl"] * sample["cy"]) / sample["dist2"]
        wgt = r["area"] * (TWO31 / r["q"].astype(F))
        gw = geom * wgt
        term = ((diff * INV_PI) * r["radiance"]) * gw[:, None]
        used = sample["traced"] if mask is None else sample["traced"] & (np.asarray(mask).reshape(-1) != 0)
        return np.where(used[:, None], term, F(0)).astype(F)


def emitter_direct(surface_rows, hit, sample, mask=None, base=None):
    """mrt_light_emitter_surfaces for N records: rgba [N, 4].  base None: written ({0 + term, 1} for a hit, zeros for a miss); base [N,
    4]: MRT_EMITTER_ACCUMULATE into it (rgb = base + term for a hit, the rest kept)."""
    hit = np.asarray(hit, dtype=bool)
    term = emitter_terms(surface_rows, sample, mask)
    with np.errstate(all="ignore"):
        if base is None:
            out = np.zeros((hit.shape[0], 4), F)
            out[hit, :3] = F(0) + term[hit]
            out[hit, 3] = 1
        else:
            out = np.asarray(base, dtype=F).copy()
            out[hit, :3] = out[hit, :3] + term[hit]
    return out


def step_emits(bounce, prev_lobe, n):
    """Where mrt_path_step_emitters runs the emission line: everywhere at bounce 0, then where the ray came from the specular lobe."""
    return np.ones(n, bool) if bounce == 0 else np.asarray(prev_lobe) == B.LOBE_SPECULAR


def path_step_emitters(state, rows, hit, nrm, in_dirs, direct, env, pixel_index, frame, bounce, max_bounces, prev_lobe, **kw):
    """mrt_path_step_emitters: path.path_step with the emission line under step_emits."""
    return P.path_step(state, rows, hit, nrm, in_dirs, direct, env, pixel_index, frame, bounce, max_bounces,
                       emits=step_emits(bounce, prev_lobe, state.shape[0]), **kw)


INV_1009 = pow(1009, -1, 1 << 32)


def frame_pixels(pixel_index, frames, frame0=0):
    """Pixel indices [len(frames) * N] whose streams under frame `frame0` are those of pixel_index under each of `frames`: the seed is
    pixel * 1009 + frame * 6529 + 7 modulo 2^32 and 1009 is odd, so (frame - frame0) * 6529 / 1009 is a pixel offset.  Many frames of a
    small grid then go through the restatements as one batch of records."""
    pixel_index = np.asarray(pixel_index, dtype=np.uint64)
    off = [((int(f) - int(frame0)) * 6529 * INV_1009) & H.M32 for f in frames]
    return np.concatenate([(pixel_index + np.uint64(o)) & np.uint64(H.M32) for o in off])


def frame_loop(trace, occluded, rays, shade_fn, env, pixel_index, frame, max_bounces, table=None, t_max=F(1e30)):
    """The renderer's loop in numpy for N primary rays (mrt_ray32): per bounce trace -> resolve -> (emitter shadows -> emitter light) ->
    step -> bounce rays, with no analytic lights.  trace(rays) returns mrt_hit32 records, occluded(rays, traced) [N] bool; shade_fn(rays,
    hits) returns (rows, pairs, shading normals) as surface.resolve does.  table = (rows, cdf): the loop samples emitters and steps with
    mrt_path_step_emitters; None: the loop of mrt_path_step, which finds emitters by chance.  Returns the final T.PATH_STATE [N]."""
    n = rays.shape[0]
    state = P.init_state(n)
    select, lobe = None, None
    for b in range(max_bounces + 1):
        hits = trace(rays)
        hit = hits["prim_id"] != -1
        if select is not None:
            hit &= select != 0   # (an entry without a ray carries the placeholder's record: a miss of an ended path)
        srows, pairs, sn = shade_fn(rays, hits)
        pos = (rays["origin"] + rays["direction"] * hits["t"][:, None]).astype(F)
        direct = np.zeros((n, 4), F)
        if table is not None and b == max_bounces:   # (that sample's light is the emission of bounce max_bounces + 1, which no loop reaches)
            state, select, lobe, active = path_step_emitters(state, srows, hit, sn, rays["direction"], direct, env, pixel_index, frame, b,
                                                             max_bounces, lobe)
        elif table is not None:
            s = emitter_samples(rays["direction"], pos, sn, hit, pixel_index, frame, T.path_emitter_draw(b), table[0], table[1], select)
            mask = (~(s["traced"] & occluded(s["rays"], s["traced"]))).astype(np.uint8)
            direct = emitter_direct(srows, hit, s, mask)
            state, select, lobe, active = path_step_emitters(state, srows, hit, sn, rays["direction"], direct, env, pixel_index, frame, b,
                                                             max_bounces, lobe)
        else:
            state, select, lobe, active = P.path_step(state, srows, hit, sn, rays["direction"], direct, env, pixel_index, frame, b, max_bounces)
        if active == 0 or b == max_bounces:
            break
        rays, _, _ = B.bounce_rays(rays["direction"], pos, sn, hit, pixel_index, frame, P.first_draw(b), t_max, pairs[:, 0], pairs[:, 1], select)
    return state
