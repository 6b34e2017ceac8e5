"""Next-event estimation with one light per record, as include/mrt_hip.h states it (mrt_cast_selected_shadows,
mrt_light_selected_surfaces), restated in numpy from what the other restatements hold: the stream and its jump (hemisphere.py), the shadow
ray (shadow.py), one light's term (lighting.py).  The only rule of its own is the choice: draw select_draw of the pixel's stream, modulo
the number of lights.  Test and tool plumbing (tests/test_selected_nee_*.py): the device's bytes and words must equal these."""
import numpy as np

from . import hemisphere as H
from . import lighting as Lg
from . import path as P
from . import shadow as Sh
from . import types as T

F = np.float32


def select_lights(pixel_index, frame, select_draw, n_lights, hit, select=None):
    """d_out_light of mrt_cast_selected_shadows for N records: the output word of draw select_draw of each pixel's stream (seeded as
    mrt_cast_bounce seeds it), modulo n_lights in uint32; T.LIGHT_NONE for a miss or a record with select == 0.  uint8 [N]."""
    hit = np.asarray(hit, dtype=bool)
    on = hit if select is None else hit & (np.asarray(select) != 0)
    out = H.draw(P.stream_seed(pixel_index, frame), select_draw).astype(np.uint32)
    k = (out % np.uint32(n_lights)).astype(np.uint8)
    return np.where(on, k, np.uint8(T.LIGHT_NONE)).astype(np.uint8)


def selected_shadow_rays(pos, nrm, hit, lights, light):
    """The ray of every record to the light it selected (mrt_ray32; the placeholder where none is traced) and which records are traced:
    shadow.shadow_rays' ray of the pair (light[i], i).  pos, nrm: (N, 3) float32; hit: (N,) bool; lights: mrt_light rows; light: (N,)
    bytes as select_lights returns them."""
    light = np.asarray(light, dtype=np.uint8)
    n = light.shape[0]
    rays = np.repeat(Sh.PLACEHOLDER, n)
    traced = np.zeros(n, bool)
    if len(lights):
        all_rays, all_traced = Sh.shadow_rays(pos, nrm, hit, lights)
        on = light < len(lights)
        at = light[on].astype(np.int64) * n + np.nonzero(on)[0]
        rays[on], traced[on] = all_rays[at], all_traced[at]
    return rays, traced


def selected_terms(rows, p, d, lights, light, mask=None, cos_outer=None):
    """The selected light's term of N hit surfaces before the scaling: rgb.c = 0 + term_k.c, or 0 where light[i] >= n_lights, the mask
    byte is 0 or lighting.light_term skips the light.  Returns (rgb [N, 3], used [N]: a term was added)."""
    lights = Lg.shade_lights(lights)
    p, v = np.asarray(p, dtype=F), Lg.view_dir(d)
    light = np.asarray(light, dtype=np.uint8)
    lit = np.ones(light.shape[0], bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    rgb = np.zeros((rows.shape[0], 3), F)
    used = np.zeros(rows.shape[0], bool)
    with np.errstate(all="ignore"):
        for k in range(lights.shape[0]):
            at = np.nonzero((light == k) & lit)[0]
            if not at.size:
                continue
            c, active, _, _ = Lg.light_term(rows[at], p[at], v[at], lights[k], None, None if cos_outer is None else cos_outer[k])
            rgb[at[active]] = F(0) + c[active]
            used[at[active]] = True
    return rgb, used


def selected_direct(rows, p, d, lights, light, mask=None, env=None, hit=None, cos_outer=None, panorama=None):
    """mrt_light_selected_surfaces for N records: rows as mrt_resolve_surfaces wrote them, p [N, 3] positions (used for hits), d [N, 3]
    incoming directions, lights T.SHADE_LIGHT rows, light [N] bytes (select_lights), mask [N] bytes or None (lit), env one T.ENVIRONMENT
    row or None, hit [N] bool (None: every record is a hit), panorama as lighting.shade_linear takes it.  Returns rgba [N, 4] float32:
    with env None, what mrt_path_step takes as d_direct."""
    N = rows.shape[0]
    hit = np.ones(N, bool) if hit is None else np.asarray(hit, dtype=bool)
    lights = Lg.shade_lights(lights)
    out = np.zeros((N, 4), F)
    idx = np.nonzero(hit)[0]
    r = rows[idx]
    rgb, _ = selected_terms(r, np.asarray(p, dtype=F)[idx], np.asarray(d, dtype=F)[idx], lights, np.asarray(light)[idx],
                            None if mask is None else np.asarray(mask).reshape(-1)[idx], cos_outer)
    with np.errstate(all="ignore"):
        rgb = (rgb * F(lights.shape[0])).astype(F)
    if env is not None:
        rgb = Lg.add_environment(rgb, r, env, panorama)
        out[~hit, :3] = Lg.miss_sky(np.asarray(d, dtype=F)[~hit], env, panorama)
    out[idx, :3] = rgb
    out[idx, 3] = 1
    return out
