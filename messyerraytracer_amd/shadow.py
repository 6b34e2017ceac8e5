"""The shadow ray of include/mrt_hip.h (mrt_cast_shadows; the reference's _trace_shadow_rays, ray_renderer.cpp:584-610) restated in
numpy: float32, one operation at a time, in the order the header states.  Test and tool plumbing (tests/test_shadow_*.py,
tests/test_source_edges_gpu.py): the device's lit masks must equal these rays traced by the oracle, byte for byte, and the rays
themselves equal what the reference's own text made of the same inputs (tests/golden/shadow_reference.npz)."""
import numpy as np

from . import types as T

F = np.float32
SHADOW_BIAS = F(1e-3)
DIR_LIGHT_MAX_DIST = F(1000.0)
MIN_DIST = F(1e-6)
PLACEHOLDER = np.zeros(1, dtype=T.RAY32)  # the reference's Ray(0, (0, 1, 0), 0, 0) for pairs it does not trace
PLACEHOLDER["direction"] = (0.0, 1.0, 0.0)


def shadow_rays(pos, nrm, hit, lights):
    """The rays of all (light, record) pairs, light-major (mrt_ray32; the placeholder where a pair is not traced), and which pairs are
    traced.  pos, nrm: (n, 3) float32; hit: (n,) bool; lights: mrt_light rows."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):  # (the position of a miss is not used)
        return _shadow_rays(np.asarray(pos, dtype=F), np.asarray(nrm, dtype=F), np.asarray(hit, dtype=bool), lights)


def _shadow_rays(pos, nrm, hit, lights):
    org = pos + nrm * SHADOW_BIAS
    rays = np.zeros((len(lights), pos.shape[0]), dtype=T.RAY32)
    traced = np.zeros(rays.shape, dtype=bool)
    for l, L in enumerate(lights):
        r = rays[l]
        r["origin"] = org
        if L["type"] == T.LIGHT_DIRECTIONAL:
            r["direction"] = L["direction"].astype(F)
            r["t_max"] = DIR_LIGHT_MAX_DIST
            ok = np.ones(pos.shape[0], dtype=bool)
        else:
            to = L["position"].astype(F)[None, :] - org
            dist = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2])
            ok = ~(dist < MIN_DIST)
            r["direction"] = to / dist[:, None]
            r["t_max"] = dist
        traced[l] = hit & (L["cast_shadows"] != 0) & ok
        r[~traced[l]] = PLACEHOLDER[0]
    return rays.reshape(-1), traced.reshape(-1)
