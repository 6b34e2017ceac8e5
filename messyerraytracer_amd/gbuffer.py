"""The reflection effect's first pass from a rasteriser's G-buffer as include/mrt_hip.h states it (mrt_cast_gbuffer_reflections,
mrt_reflection_image; rt_reflections.comp.glsl:276-332) restated in numpy: float32, one operation at a time, in the order the header
states, with decode_guide and normalize3 taken from denoise.py.  It is the standard the device is held to (tests/test_gbuffer_*.py,
tools/bench_gbuffer_reflection_frame.py): the device's rays and records must equal these rays traced by the oracle, and the image
these pixels, byte for byte.  The ctypes wrappers of the two calls are here too, and a perspective camera for tests and tools."""
import ctypes as C

import numpy as np

from . import capi
from . import types as T
from .denoise import NORMAL_OCTAHEDRAL, NORMAL_WORLD, decode_guide, max_of, normalize3  # noqa: F401
from .reflection import NORMAL_OFFSET, PLACEHOLDER, PLACEHOLDER_HIT  # noqa: F401

F = np.float32
D = np.float64
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


class GBufferDesc(C.Structure):
    """mrt_gbuffer"""
    _fields_ = [("struct_size", C.c_uint32), ("normal_kind", C.c_uint32), ("inv_projection", C.c_float * 16), ("inv_view", C.c_float * 16),
                ("roughness_threshold", C.c_float), ("max_distance", C.c_float), ("d_depth", C.c_void_p), ("d_normal_roughness", C.c_void_p)]


class GBuffer:
    """A frame's G-buffer on the host: depth [H * W] and normal_roughness [H * W, 4] float32, the two matrices as 16 floats each,
    column-major (m[4 c + r] = column c, row r), and the effect's two parameters."""

    def __init__(self, depth, normal_roughness, inv_projection, inv_view, normal_kind=NORMAL_OCTAHEDRAL, roughness_threshold=0.3,
                 max_distance=25.0):
        self.depth = np.ascontiguousarray(depth, dtype=F).reshape(-1)
        self.normal_roughness = np.ascontiguousarray(normal_roughness, dtype=F).reshape(-1, 4)
        self.inv_projection = np.asarray(inv_projection, dtype=F).reshape(16).copy()
        self.inv_view = np.asarray(inv_view, dtype=F).reshape(16).copy()
        self.normal_kind, self.roughness_threshold, self.max_distance = int(normal_kind), F(roughness_threshold), F(max_distance)

    def desc(self, d_depth, d_normal_roughness):
        """mrt_gbuffer with the images at these device pointers"""
        g = GBufferDesc()
        g.struct_size, g.normal_kind = C.sizeof(GBufferDesc), self.normal_kind
        g.inv_projection[:] = [float(x) for x in self.inv_projection]
        g.inv_view[:] = [float(x) for x in self.inv_view]
        g.roughness_threshold, g.max_distance = float(self.roughness_threshold), float(self.max_distance)
        g.d_depth = None if d_depth is None else int(d_depth)
        g.d_normal_roughness = None if d_normal_roughness is None else int(d_normal_roughness)
        return g


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _matrix(m):
    """m[k] of one matrix [16] or of one per texel [n, 16], ready to broadcast against [n]"""
    m = np.asarray(m, dtype=F).reshape(-1, 16)
    return [m[:, k] if m.shape[0] > 1 else m[0, k] for k in range(16)]


def texel_surface(kind, P, V, x, y, w, h, depth, guide):
    """Per texel: (world [n, 3], d [n, 3], n [n, 3], roughness [n]).  x, y, w, h: integers per texel or one for all; P, V: [16] or [n, 16]."""
    depth = np.asarray(depth, dtype=F).reshape(-1)
    P, V = _matrix(P), _matrix(V)
    nx, ny, nz, rough = decode_guide(kind, np.asarray(guide, dtype=F).reshape(-1, 4))
    u = (np.asarray(x, dtype=np.uint32).astype(F) + F(0.5)) / np.asarray(w, dtype=np.uint32).astype(F)
    v = (np.asarray(y, dtype=np.uint32).astype(F) + F(0.5)) / np.asarray(h, dtype=np.uint32).astype(F)
    cx = u * F(2) - F(1)
    cy = v * F(2) - F(1)
    q0 = ((P[0] * cx + P[4] * cy) + P[8] * depth) + P[12]
    q1 = ((P[1] * cx + P[5] * cy) + P[9] * depth) + P[13]
    q2 = ((P[2] * cx + P[6] * cy) + P[10] * depth) + P[14]
    q3 = ((P[3] * cx + P[7] * cy) + P[11] * depth) + P[15]
    vx = q0 / q3
    vy = q1 / q3
    vz = q2 / q3
    wx = ((V[0] * vx + V[4] * vy) + V[8] * vz) + V[12]
    wy = ((V[1] * vx + V[5] * vy) + V[9] * vz) + V[13]
    wz = ((V[2] * vx + V[6] * vy) + V[10] * vz) + V[14]
    dx = wx - V[12]
    dy = wy - V[13]
    dz = wz - V[14]
    dx, dy, dz = normalize3(dx, dy, dz)
    n = depth.shape[0]
    full = lambda *c: np.stack([np.broadcast_to(np.asarray(a, dtype=F), (n,)) for a in c], axis=1)  # noqa: E731
    return full(wx, wy, wz), full(dx, dy, dz), full(nx, ny, nz), np.broadcast_to(rough, (n,)).astype(F)


def texel_rays(kind, P, V, roughness_threshold, max_distance, x, y, w, h, depth, guide):
    """(rays, traced): mrt_ray32 per texel (the placeholder where traced is false)"""
    depth = np.asarray(depth, dtype=F).reshape(-1)
    thr = np.asarray(roughness_threshold, dtype=F)
    with np.errstate(**_QUIET):
        world, d, n, rough = texel_surface(kind, P, V, x, y, w, h, depth, guide)
        k = F(2) * ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2])
        dirs = d - k[:, None] * n
        org = world + n * NORMAL_OFFSET
        finite = np.isfinite(org).all(axis=1) & np.isfinite(dirs).all(axis=1)
        traced = (depth < F(1)) & (rough <= thr) & finite
    rays = np.zeros(depth.shape[0], dtype=T.RAY32)
    rays["origin"], rays["direction"] = org, dirs
    rays["t_min"], rays["t_max"] = F(0), np.asarray(max_distance, dtype=F)
    rays[~traced] = PLACEHOLDER[0]
    return rays, traced


def texel_image(kind, P, V, roughness_threshold, x, y, w, h, depth, guide, prim_id, hit_normal, lit=None):
    """The reflection image's pixels [n, 4] from the rays' records"""
    depth = np.asarray(depth, dtype=F).reshape(-1)
    thr = np.asarray(roughness_threshold, dtype=F)
    hn = np.asarray(hit_normal, dtype=F).reshape(-1, 3)
    with np.errstate(**_QUIET):
        _, d, _, rough = texel_surface(kind, P, V, x, y, w, h, depth, guide)
        ndotl = max_of((hn[:, 0] * -d[:, 0] + hn[:, 1] * -d[:, 1]) + hn[:, 2] * -d[:, 2], F(0))
        grey = F(0.5) + F(0.5) * ndotl
        conf = F(1) - rough / thr
    out = np.stack([grey, grey, grey, conf], axis=1).astype(F)
    if lit is not None:
        out[:, :3] = np.asarray(lit, dtype=F).reshape(-1, 4)[:, :3]
    out[np.asarray(prim_id).reshape(-1) == -1] = F(0)
    return out


def _pixels(w, h):
    i = np.arange(w * h, dtype=np.uint64)
    return (i % np.uint64(w)).astype(np.uint32), (i // np.uint64(w)).astype(np.uint32)


def gbuffer_rays(g, w, h):
    """mrt_cast_gbuffer_reflections' rays of a w x h frame: (rays [w * h] mrt_ray32, traced [w * h] bool)"""
    x, y = _pixels(w, h)
    return texel_rays(g.normal_kind, g.inv_projection, g.inv_view, g.roughness_threshold, g.max_distance, x, y, w, h, g.depth, g.normal_roughness)


def reflection_image(g, w, h, hits, lit=None):
    """mrt_reflection_image: [w * h, 4] float32 from the T.HIT32 records of the cast; lit: [w * h, 4] or None"""
    x, y = _pixels(w, h)
    return texel_image(g.normal_kind, g.inv_projection, g.inv_view, g.roughness_threshold, x, y, w, h, g.depth, g.normal_roughness,
                       hits["prim_id"], hits["normal"], lit)


# ---- a perspective camera for tests and tools -------------------------------------------------------------------------------------
def octahedral_encode(n):
    """Godot's octahedral_encode of unit normals [n, 3] -> [n, 2] in [0, 1], float64 rounded once (test inputs, not a pinned formula)"""
    n = np.asarray(n, dtype=D)
    s = np.abs(n).sum(axis=1, keepdims=True)
    p = n[:, :2] / np.where(s == 0, 1.0, s)
    fold = (1.0 - np.abs(p[:, ::-1])) * np.where(p >= 0, 1.0, -1.0)
    p = np.where(n[:, 2:3] < 0, fold, p)
    return (p * 0.5 + 0.5).astype(F)


class Camera:
    """A perspective camera whose clip depth runs from 0 at `near` to 1 at `far`, looking down its own -z with +y of clip space along
    `up` turned into image rows (pixel row 0 is clip y = -1).  projection and view are float64; inv_projection and inv_view are their
    float64 inverses rounded once to float32, 16 floats each, column-major."""

    def __init__(self, origin, target, up=(0.0, 1.0, 0.0), fov_y=60.0, aspect=1.0, near=0.1, far=100.0):
        o, t, up = (np.asarray(a, dtype=D) for a in (origin, target, up))
        f = (t - o) / np.linalg.norm(t - o)
        r = np.cross(f, up)
        r /= np.linalg.norm(r)
        u = np.cross(r, f)
        cam_to_world = np.eye(4)
        cam_to_world[:3, 0], cam_to_world[:3, 1], cam_to_world[:3, 2], cam_to_world[:3, 3] = r, u, -f, o
        self.origin, self.near, self.far = o, float(near), float(far)
        self.view = np.linalg.inv(cam_to_world)
        k = 1.0 / np.tan(np.radians(fov_y) / 2.0)
        self.projection = np.array([[k / aspect, 0, 0, 0], [0, k, 0, 0], [0, 0, far / (near - far), near * far / (near - far)], [0, 0, -1, 0]], dtype=D)
        self.inv_view = cam_to_world.T.reshape(-1).astype(F)                       # [4 c + r]
        self.inv_projection = np.linalg.inv(self.projection).T.reshape(-1).astype(F)

    def primary_rays(self, w, h, t_max=1e30):
        """mrt_ray32 through the pixel centres (float64, rounded once), row-major"""
        x, y = _pixels(w, h)
        cx, cy = (x.astype(D) + 0.5) / w * 2 - 1, (y.astype(D) + 0.5) / h * 2 - 1
        inv = np.linalg.inv(self.projection @ self.view)
        p = np.stack([cx, cy, np.full_like(cx, 0.5), np.ones_like(cx)], axis=1) @ inv.T
        d = p[:, :3] / p[:, 3:4] - self.origin
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.zeros(w * h, dtype=T.RAY32)
        rays["origin"], rays["direction"], rays["t_min"], rays["t_max"] = self.origin.astype(F), d.astype(F), F(0), F(t_max)
        return rays

    def view_z(self, points):
        """the camera-space z of world points [n, 3] (negative in front), float64"""
        return np.asarray(points, dtype=D) @ self.view[2, :3] + self.view[2, 3]

    def depth(self, points):
        """the clip depth of world points [n, 3], float64 (not clamped)"""
        z = self.view_z(points)
        with np.errstate(**_QUIET):
            return (self.projection[2, 2] * z + self.projection[2, 3]) / -z


# ---- the calls (ctx: a capi.Context; images and records: device pointers) ----------------------------------------------------------
_BOUND = []


def lib():
    L = capi.load()
    if not _BOUND:
        P, V, U = C.POINTER(GBufferDesc), C.c_void_p, C.c_uint32
        L.mrt_cast_gbuffer_reflections.argtypes = [V, P, U, U, V, V, U, U]
        L.mrt_reflection_image.argtypes = [V, P, U, U, V, V, V, U]
        _BOUND.append(True)
    return L


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def cast_gbuffer_reflections(ctx, desc, w, h, d_out_hits, d_out_rays=None, query_mask=0xFFFFFFFF, flags=0):
    ctx._chk(lib().mrt_cast_gbuffer_reflections(ctx.h, C.byref(desc), w, h, _p(d_out_hits), _p(d_out_rays), query_mask, flags))


def reflection_image_device(ctx, desc, w, h, d_hits, d_reflection, d_lit=None, flags=0):
    ctx._chk(lib().mrt_reflection_image(ctx.h, C.byref(desc), w, h, _p(d_hits), _p(d_lit), _p(d_reflection), flags))


assert C.sizeof(GBufferDesc) == 160
