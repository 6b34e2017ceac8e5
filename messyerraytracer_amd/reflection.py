"""The mirror-reflection ray of include/mrt_hip.h (mrt_cast_reflections; rt_reflections.comp.glsl:307-313 with the normal faced
against the incoming ray) restated in numpy: float32, one operation at a time, in the order the header states.  Test and tool
plumbing (tests/test_reflections_*.py, tests/test_source_edges_gpu.py): the device's rays and records must equal these rays traced by
the oracle, byte for byte.  The direction is GLSL's reflect, whose rounding the reference leaves open: tests/test_reflections_cpu.py
holds it to float64 within a derived bound."""
import numpy as np

from . import types as T

F = np.float32
NORMAL_OFFSET = F(0.01)
PLACEHOLDER = np.zeros(1, dtype=T.RAY32)  # the reference's Ray(0, (0, 1, 0), 0, 0) for records without a ray
PLACEHOLDER["direction"] = (0.0, 1.0, 0.0)
PLACEHOLDER_HIT = np.zeros(1, dtype=T.HIT32)  # what mrt_cast writes for it: t = t_max = 0, a miss
PLACEHOLDER_HIT["prim_id"] = -1


def reflection_rays(dirs, pos, nrm, traced, max_distance):
    """(rays, flipped): mrt_ray32 per record (the placeholder where traced is false) and whether the normal was turned.
    dirs, pos, nrm: (n, 3) float32; traced: (n,) bool."""
    dirs, pos, traced = np.asarray(dirs, dtype=F), np.asarray(pos, dtype=F), np.asarray(traced, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):  # (the position of a miss is not used)
        dx, dy, dz = dirs[:, 0], dirs[:, 1], dirs[:, 2]
        n = np.asarray(nrm).astype(F).copy()
        c = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2] * dz
        flip = c > F(0)
        n[flip] = -n[flip]
        k = F(2) * ((n[:, 0] * dx + n[:, 1] * dy) + n[:, 2] * dz)
        rays = np.zeros(dirs.shape[0], dtype=T.RAY32)
        rays["direction"] = np.stack([dx - k * n[:, 0], dy - k * n[:, 1], dz - k * n[:, 2]], axis=1)
        rays["origin"] = pos + n * NORMAL_OFFSET
        rays["t_min"], rays["t_max"] = F(0), F(max_distance)
    rays[~traced] = PLACEHOLDER[0]
    return rays, flip & traced
