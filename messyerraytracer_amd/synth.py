"""Deterministic synthetic scenes and ray batches.

Only IEEE-exact operations (+ - * / sqrt on float32, integer mixing) are used,
so the same arrays come out on every machine: the golden fixtures made in the
build container and the inputs regenerated on the GPU box are bit-identical.

PRNG: splitmix64 used as a counter-based generator; draw k of stream `seed` is
mix(seed + (k+1)*GAMMA); uniform float32 in [0,1) from the top 24 bits.
"""
import numpy as np

from .types import RAY32, FLT_MAX

_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed: int, start: int, count: int) -> np.ndarray:
    """Draws start .. start+count-1 of stream `seed` as uint64."""
    with np.errstate(over="ignore"):
        k = np.arange(start + 1, start + count + 1, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + k * _GAMMA
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return z


def uniform01(seed: int, start: int, count: int) -> np.ndarray:
    """float32 uniforms in [0,1): top 24 bits * 2^-24 (exact)."""
    return (splitmix64(seed, start, count) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def _soup_block(n: int, s: float, seed: int, start_tri: int) -> np.ndarray:
    u = uniform01(seed, start_tri * 12, n * 12).reshape(n, 12)
    c = u[:, 0:3] * np.float32(10.0) - np.float32(5.0)
    off = (u[:, 3:12] * np.float32(2.0) - np.float32(1.0)) * np.float32(s)
    return (c[:, None, :] + off.reshape(n, 3, 3)).astype(np.float32)


def soup(n_tris: int, s: float, seed: int) -> np.ndarray:
    """Soup(N, s, seed): centre c ~ U[-5,5]^3, vertices c + U[-s,s]^3.
    Returns (n,3,3) float32.  Degenerate triangles (|e1 x e2|^2 < 1e-12) are
    redrawn from stream seed + 0x51ED270B."""
    out = np.empty((n_tris, 3, 3), dtype=np.float32)
    step = 1 << 20
    for a in range(0, n_tris, step):
        b = min(n_tris, a + step)
        out[a:b] = _soup_block(b - a, s, seed, a)
    redraw_seed, rnd = seed + 0x51ED270B, 0
    while True:
        e1 = out[:, 1] - out[:, 0]
        e2 = out[:, 2] - out[:, 0]
        cr = np.cross(e1.astype(np.float64), e2.astype(np.float64))
        bad = np.nonzero((cr * cr).sum(axis=1) < 1e-12)[0]
        if bad.size == 0:
            return out
        out[bad] = _soup_block(bad.size, s, redraw_seed, rnd)
        rnd += bad.size


def cube() -> np.ndarray:
    """Unit cube at the origin, 12 triangles, outward winding (config C1)."""
    p = np.array([[-.5, -.5, -.5], [.5, -.5, -.5], [.5, .5, -.5], [-.5, .5, -.5],
                  [-.5, -.5, .5], [.5, -.5, .5], [.5, .5, .5], [-.5, .5, .5]], dtype=np.float32)
    quads = [(4, 5, 6, 7), (1, 0, 3, 2), (5, 1, 2, 6), (0, 4, 7, 3), (7, 6, 2, 3), (0, 1, 5, 4)]
    tris = []
    for a, b, c, d in quads:
        tris.append([p[a], p[b], p[c]])
        tris.append([p[a], p[c], p[d]])
    return np.asarray(tris, dtype=np.float32)


def _unit_vectors(seed: int, n: int, dims: int) -> np.ndarray:
    """n uniformly distributed unit vectors in `dims` dimensions by rejection
    from the cube (8 candidates per round), float32, IEEE-exact ops only."""
    out = np.zeros((n, dims), dtype=np.float32)
    k = 8
    step = 1 << 19
    for a in range(0, n, step):
        b = min(n, a + step)
        todo = np.arange(a, b)
        rnd = 0
        while todo.size:
            # vector i of round rnd uses draws [i*k*dims, (i+1)*k*dims) of stream seed + rnd*7919
            u = uniform01(seed + rnd * 7919, a * k * dims, (b - a) * k * dims).reshape(b - a, k, dims)[todo - a]
            p = u * np.float32(2.0) - np.float32(1.0)
            l2 = (p * p).sum(axis=2, dtype=np.float32)
            ok = (l2 <= np.float32(1.0)) & (l2 >= np.float32(1e-4))
            first = ok.argmax(axis=1)
            has = ok.any(axis=1)
            rows = np.arange(todo.size)
            sel = p[rows, first]
            ln = np.sqrt(l2[rows, first])
            vec = (sel / ln[:, None]).astype(np.float32)
            out[todo[has]] = vec[has]
            todo = todo[~has]
            rnd += 1
    return out


def incoherent_rays(m: int, seed: int = 7, extent: float = 6.0) -> np.ndarray:
    """Incoherent(M, seed): origin ~ U[-extent,extent]^3, direction uniform on
    the sphere; t_min = 0.001, t_max = FLT_MAX (Ray() defaults, src/core/ray.h:59)."""
    rays = np.zeros(m, dtype=RAY32)
    u = uniform01(seed, 0, m * 3).reshape(m, 3)
    rays["origin"] = u * np.float32(2.0 * extent) - np.float32(extent)
    d = _unit_vectors(seed + 0x0DD5EED, m, 3)
    # renormalise once in float32 so |d| is as close to 1 as float32 allows
    l = np.sqrt((d * d).sum(axis=1, dtype=np.float32))
    rays["direction"] = (d / l[:, None]).astype(np.float32)
    rays["t_min"] = np.float32(0.001)
    rays["t_max"] = FLT_MAX
    return rays


def incoherent_rays_at(index: np.ndarray, seed: int = 7, extent: float = 6.0) -> np.ndarray:
    """Rays index[0], index[1], ... of incoherent_rays(m, seed, extent) for any m > max(index), without generating the
    whole batch (the generator is counter based: ray i takes draws [3 i, 3 i + 3) of the origin stream and draws
    [24 i, 24 i + 24) of each rejection round of the direction stream).  Same arithmetic, same bits."""
    index = np.asarray(index, dtype=np.int64)
    rays = np.zeros(index.shape[0], dtype=RAY32)
    d = np.zeros((index.shape[0], 3), dtype=np.float32)
    for j, i in enumerate(index):
        i = int(i)
        u = uniform01(seed, i * 3, 3)
        rays["origin"][j] = u * np.float32(2.0 * extent) - np.float32(extent)
        rnd = 0
        while True:   # _unit_vectors(seed + 0x0DD5EED, m, 3), element i: first of 8 candidates per round inside the unit ball
            c = uniform01(seed + 0x0DD5EED + rnd * 7919, i * 24, 24).reshape(8, 3) * np.float32(2.0) - np.float32(1.0)
            l2 = (c * c).sum(axis=1, dtype=np.float32)
            ok = (l2 <= np.float32(1.0)) & (l2 >= np.float32(1e-4))
            if ok.any():
                k = int(ok.argmax())
                d[j] = (c[k] / np.sqrt(l2[k])).astype(np.float32)
                break
            rnd += 1
    l = np.sqrt((d * d).sum(axis=1, dtype=np.float32))
    rays["direction"] = (d / l[:, None]).astype(np.float32)
    rays["t_min"] = np.float32(0.001)
    rays["t_max"] = FLT_MAX
    return rays


def multi_mesh(n_meshes: int = 64, tris_per_mesh: int = 156250, s: float = 0.025, seed: int = 100):
    """Config C5: n_meshes soups, each scaled into a cell of a 4x4x4 lattice
    spanning [-5,5]^3 with a seeded rigid rotation, flattened to world space
    with running triangle ids (raytracer_server.cpp:700-711 semantics).
    Returns (verts (N,3,3) float32, mesh_of_tri (N,) uint32)."""
    side = 4
    cell = np.float32(10.0 / side)
    scale = np.float32(0.24)          # [-5,5] -> [-1.2,1.2]: a 2.4-unit cell
    verts = np.empty((n_meshes * tris_per_mesh, 3, 3), dtype=np.float32)
    mesh_id = np.empty(n_meshes * tris_per_mesh, dtype=np.uint32)
    quats = _unit_vectors(seed + 0xA11CE, n_meshes, 4)
    for m in range(n_meshes):
        local = soup(tris_per_mesh, s, seed + m) * scale
        w, x, y, z = [np.float32(v) for v in quats[m]]
        two = np.float32(2.0)
        one = np.float32(1.0)
        rot = np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                        [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                        [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=np.float32)
        lattice = m % (side ** 3)
        cx = np.float32(-5.0) + cell * np.float32((lattice % side) + 0.5)
        cy = np.float32(-5.0) + cell * np.float32(((lattice // side) % side) + 0.5)
        cz = np.float32(-5.0) + cell * np.float32((lattice // (side * side)) + 0.5)
        p = local.reshape(-1, 3)
        wx = p[:, 0] * rot[0, 0] + p[:, 1] * rot[0, 1] + p[:, 2] * rot[0, 2] + cx
        wy = p[:, 0] * rot[1, 0] + p[:, 1] * rot[1, 1] + p[:, 2] * rot[1, 2] + cy
        wz = p[:, 0] * rot[2, 0] + p[:, 1] * rot[2, 1] + p[:, 2] * rot[2, 2] + cz
        a = m * tris_per_mesh
        verts[a:a + tris_per_mesh] = np.stack([wx, wy, wz], axis=1).reshape(-1, 3, 3)
        mesh_id[a:a + tris_per_mesh] = m
    return verts, mesh_id


def multi_mesh_instances(n_meshes: int = 64, tris_per_mesh: int = 156250, s: float = 0.025, seed: int = 100):
    """The same scene as multi_mesh() before flattening: mesh-space vertices (n_meshes*tris_per_mesh,3,3)
    and one types.INSTANCE per mesh (rotation + lattice-cell origin), the input of
    mrt_build_instanced_scene_device.  flatten_instances(*multi_mesh_instances(...)) == multi_mesh(...)[0]."""
    from . import types as T
    side = 4
    cell = np.float32(10.0 / side)
    scale = np.float32(0.24)
    local = np.empty((n_meshes * tris_per_mesh, 3, 3), dtype=np.float32)
    inst = np.zeros(n_meshes, dtype=T.INSTANCE)
    quats = _unit_vectors(seed + 0xA11CE, n_meshes, 4)
    for m in range(n_meshes):
        local[m * tris_per_mesh:(m + 1) * tris_per_mesh] = soup(tris_per_mesh, s, seed + m) * scale
        w, x, y, z = [np.float32(v) for v in quats[m]]
        two, one = np.float32(2.0), np.float32(1.0)
        rot = np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                        [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                        [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=np.float32)
        lattice = m % (side ** 3)
        inst[m]["first_tri"], inst[m]["n_tris"], inst[m]["layers"] = m * tris_per_mesh, tris_per_mesh, 0xFFFFFFFF
        inst[m]["basis"] = rot.reshape(9)
        inst[m]["origin"] = [np.float32(-5.0) + cell * np.float32((lattice % side) + 0.5),
                             np.float32(-5.0) + cell * np.float32(((lattice // side) % side) + 0.5),
                             np.float32(-5.0) + cell * np.float32((lattice // (side * side)) + 0.5)]
    return local, inst


def many_instances(n_instances: int = 65536, n_meshes: int = 4, tris_per_mesh: int = 24, extent: float = 5.0, seed: int = 11):
    """A scene of many placed copies of a few small meshes (the top level dominates): n_meshes soups of tris_per_mesh triangles,
    each placed n_instances / n_meshes times with a seeded rotation, a scale in [0.15, 0.6) and an origin in [-extent, extent]^3, so
    that instances overlap; every 64th instance is an exact duplicate of the one before it (same mesh, transform and mask: ties
    across instances, which the lower flat id wins).  Masks: one of bits 0-3 per instance.  Returns mesh-space vertices
    (n_meshes*tris_per_mesh,3,3) float32 and n_instances types.INSTANCE rows."""
    from . import types as T
    local = np.concatenate([soup(tris_per_mesh, 0.35, seed + m) * np.float32(0.2) for m in range(n_meshes)]).astype(np.float32)
    inst = np.zeros(n_instances, dtype=T.INSTANCE)
    mesh = np.arange(n_instances, dtype=np.uint32) % np.uint32(n_meshes)
    inst["first_tri"] = mesh * np.uint32(tris_per_mesh)
    inst["n_tris"] = tris_per_mesh
    u = uniform01(seed + 0xB0B, 0, 5 * n_instances).reshape(n_instances, 5)
    inst["layers"] = np.uint32(1) << (u[:, 4] * 4).astype(np.uint32)
    q = _unit_vectors(seed + 0x5CA1E, n_instances, 4).astype(np.float32)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = np.float32(1.0), np.float32(2.0)
    rot = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                    two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                    two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=1)
    scale = (np.float32(0.15) + np.float32(0.45) * u[:, 3]).astype(np.float32)
    inst["basis"] = (rot * scale[:, None]).astype(np.float32)
    inst["origin"] = (np.float32(-extent) + np.float32(2.0 * extent) * u[:, :3]).astype(np.float32)
    dup = np.arange(64, n_instances, 64)
    for f in ("first_tri", "n_tris", "layers", "basis", "origin"):
        inst[f][dup] = inst[f][dup - 1]
    return local, inst


def flatten_instances(local: np.ndarray, inst: np.ndarray) -> np.ndarray:
    """World-space vertices of every instance, in instance order: Transform3D::xform per vertex as
    RayTracerServer::_rebuild_scene applies it (raytracer_server.cpp:700-711): basis row . v summed
    left to right, plus origin, all in float32."""
    out = []
    for i in inst:
        p = local[int(i["first_tri"]):int(i["first_tri"]) + int(i["n_tris"])].reshape(-1, 3)
        b, o = i["basis"].astype(np.float32), i["origin"].astype(np.float32)
        w = [p[:, 0] * b[3 * r] + p[:, 1] * b[3 * r + 1] + p[:, 2] * b[3 * r + 2] + o[r] for r in range(3)]
        out.append(np.stack(w, axis=1).reshape(-1, 3, 3))
    return np.concatenate(out).astype(np.float32)



def _facing(tris: np.ndarray, point, towards: bool) -> np.ndarray:
    """Winds every triangle so that its normal cross(v1 - v0, v2 - v0) points towards `point` (or away from it)."""
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    side = np.einsum("ij,ij->i", np.cross(e1, e2), np.asarray(point, np.float32) - tris.mean(axis=1))
    flip = (side < 0) if towards else (side > 0)
    out = tris.copy()
    out[flip, 1], out[flip, 2] = tris[flip, 2], tris[flip, 1]
    return out


def room(subdiv: int = 29, size: float = 10.0, height: float = 6.0):
    """A shadow test scene in the shapes of the reference's demo scene (tools/generate_demo_assets.py): a closed room of
    subdivided wall quads (floor, ceiling and four walls, one mesh each, normals facing into the room), a 32 x 16 UV sphere and
    two boxes (one mesh, two instances).  Returns mesh-space vertices (n,3,3) float32 and one types.INSTANCE per placed mesh:
    the walls on layer 2, the sphere and the boxes on layer 1.  flatten_instances(*room()) is the same scene flat (11 076
    triangles with the default subdivision).  The sphere's vertices come from float64 sin / cos rounded to float32."""
    from . import types as T
    f = np.float32
    n, hs, hh = subdiv, f(size / 2), f(height)
    walls = [  # corner, u, v: the cells are corner + u * i / n + v * j / n
        ((-hs, f(0), -hs), (0, 0, size), (size, 0, 0)),     # floor
        ((-hs, hh, -hs), (size, 0, 0), (0, 0, size)),       # ceiling
        ((-hs, f(0), -hs), (0, height, 0), (0, 0, size)),   # x = -size / 2
        ((hs, f(0), -hs), (0, 0, size), (0, height, 0)),    # x = +size / 2
        ((-hs, f(0), -hs), (size, 0, 0), (0, height, 0)),   # z = -size / 2
        ((-hs, f(0), hs), (0, height, 0), (size, 0, 0)),    # z = +size / 2
    ]
    centre = (f(0), hh / f(2), f(0))
    meshes = []
    for corner, u, v in walls:
        c, u, v = np.asarray(corner, f), np.asarray(u, f), np.asarray(v, f)
        k = np.arange(n + 1, dtype=f) / f(n)
        grid = c[None, None, :] + u[None, None, :] * k[:, None, None] + v[None, None, :] * k[None, :, None]
        p00, p10, p11, p01 = grid[:-1, :-1], grid[1:, :-1], grid[1:, 1:], grid[:-1, 1:]
        quads = np.stack([np.stack([p00, p10, p11], axis=2), np.stack([p00, p11, p01], axis=2)], axis=2)
        meshes.append(_facing(quads.reshape(-1, 3, 3), centre, towards=True))
    # UV sphere, unit radius: 32 segments, 16 rings (one triangle per cell at the poles)
    th = (np.arange(17, dtype=np.float64) * np.pi / 16)[:, None]
    ph = (np.arange(33, dtype=np.float64) * 2 * np.pi / 32)[None, :]
    sp = np.stack([np.sin(th) * np.cos(ph), np.cos(th) * np.ones_like(ph), np.sin(th) * np.sin(ph)], axis=-1).astype(f)
    sphere = []
    for r in range(16):
        for q in range(32):
            a, b, c, d = sp[r, q], sp[r + 1, q], sp[r + 1, q + 1], sp[r, q + 1]
            if r != 0:
                sphere.append((a, c, d))
            if r != 15:
                sphere.append((a, b, c))
    meshes.append(_facing(np.asarray(sphere, f), (0, 0, 0), towards=False))
    meshes.append(cube())  # unit box centred on the origin (outward already)
    local = np.concatenate(meshes).astype(f)
    inst = np.zeros(9, dtype=T.INSTANCE)
    first = np.cumsum([0] + [m.shape[0] for m in meshes])
    place = [(k, 2, np.eye(3), (0, 0, 0)) for k in range(6)]
    rot = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]])  # about y, a 3-4-5 triangle
    place += [(6, 1, 1.25 * np.eye(3), (0.5, 1.25, -0.5)),            # the sphere, resting on the floor
              (7, 1, 1.5 * rot, (-2.25, 0.75, 1.25)),                 # a box of side 1.5, turned
              (7, 1, np.diag([1.0, 2.5, 1.0]), (2.5, 1.25, -2.0))]    # a pillar
    for i, (m, layers, basis, origin) in enumerate(place):
        inst[i]["first_tri"], inst[i]["n_tris"], inst[i]["layers"] = first[m], meshes[m].shape[0], layers
        inst[i]["basis"] = np.asarray(basis, f).reshape(9)
        inst[i]["origin"] = np.asarray(origin, f)
    return local, inst

def deform(verts: np.ndarray, amplitude: float, phase: float, seed: int = 0) -> np.ndarray:
    """A frame of a smooth, seeded animation of a mesh: every vertex moves by a displacement field of three sine waves
    (direction, wave vector and offset drawn from the seed), scaled by `amplitude`, travelling with `phase`.  Vertices a
    triangle shares move alike, so a closed mesh stays closed.  Evaluated in float64 and rounded once to float32: the same
    frame for the same arguments (tests and tools/bench_refit.py share the frames).  amplitude 0 returns a copy."""
    v = np.asarray(verts, dtype=np.float32)
    p = v.reshape(-1, 3).astype(np.float64)
    u = uniform01(seed ^ 0xDEF0, 0, 27).reshape(3, 9).astype(np.float64)
    d = np.zeros_like(p)
    for k in range(3):
        direction = u[k, 0:3] - 0.5
        direction /= np.linalg.norm(direction) + 1e-12
        wave = (u[k, 3:6] - 0.5) * 2.0 * np.pi * (0.5 + u[k, 6])
        d += np.sin(p @ wave + phase * (1.0 + u[k, 7]) + 2.0 * np.pi * u[k, 8])[:, None] * direction[None, :]
    return (p + (amplitude / 3.0) * d).astype(np.float32).reshape(v.shape)


# Named workloads of BASELINE.json `configs`.
CONFIGS = {
    "C1": dict(scene="cube", grid=(16, 12), origin=(0.0, 0.0, 3.0), forward=(0.0, 0.0, -1.0), fov=60.0),
    "C2": dict(scene="soup", n_tris=100_000, s=0.10, seed=1, grid=(1024, 1024),
               origin=(0.0, 0.0, -12.0), forward=(0.0, 0.0, 1.0), fov=50.0),
    "C3": dict(scene="soup", n_tris=1_000_000, s=0.05, seed=1, grid=(4096, 4096),
               origin=(0.0, 0.0, -12.0), forward=(0.0, 0.0, 1.0), fov=50.0),
    "C4": dict(scene="soup", n_tris=1_000_000, s=0.05, seed=1, incoherent=1 << 24, ray_seed=7),
    "C5": dict(scene="multi_mesh", n_meshes=64, tris_per_mesh=156_250, s=0.025, seed=100, grid=(8192, 8192),
               origin=(0.0, 0.0, -12.0), forward=(0.0, 0.0, 1.0), fov=50.0),
}


def scene_vertices(cfg: dict) -> np.ndarray:
    if cfg["scene"] == "cube":
        return cube()
    if cfg["scene"] == "soup":
        return soup(cfg["n_tris"], cfg["s"], cfg["seed"])
    if cfg["scene"] == "multi_mesh":
        return multi_mesh(cfg["n_meshes"], cfg["tris_per_mesh"], cfg["s"], cfg["seed"])[0]
    raise ValueError(cfg["scene"])
