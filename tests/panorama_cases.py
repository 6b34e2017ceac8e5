"""Images and directions of the panorama tests (test_panorama_cpu.py, test_panorama_gpu.py) and of the recording in
tests/golden/panorama_reference.npz: integer and float32 arithmetic alone, so that every machine makes the same bytes."""
import numpy as np

F = np.float32
SIZES = ((1, 1), (2, 1), (3, 2), (64, 32), (257, 129))   # (width, height) of the seeded images
SMOOTH = (96, 48)


def noise_image(width, height, seed):
    """[height, width, 4] float32, texels uniform in [0.25, 4] from a multiplicative hash of the float's index (never dark: a
    relative difference is never taken against a small result); alpha carries the same noise and is never read"""
    i = np.arange(width * height * 4, dtype=np.uint64)
    h = ((i + np.uint64(seed)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    k = (h >> np.uint64(8)).astype(F) * F(2.0 ** -24)   # exact
    return (k * F(3.75) + F(0.25)).astype(F).reshape(height, width, 4)


def smooth_image():
    """a smooth, cyclic-in-x image in [0.5, 3.5]: products of float32 polynomials of the texel's coordinates"""
    w, h = SMOOTH
    x = ((np.arange(w, dtype=F) + F(0.5)) / F(w))[None, :]
    y = ((np.arange(h, dtype=F) + F(0.5)) / F(h))[:, None]
    bump = (F(4) * x) * (F(1) - x)              # 0 at both ends of a row, 1 in the middle
    img = np.zeros((h, w, 4), F)
    img[..., 0] = F(0.5) + (F(3) * bump) * (F(1) - y)
    img[..., 1] = F(0.5) + (F(3) * y) * (F(1) - bump * F(0.5))
    img[..., 2] = F(0.5) + (F(3) * (bump * bump)) * y
    img[..., 3] = 1
    return img


def images():
    """name -> image, in the recording's order"""
    out = {"%dx%d" % s: noise_image(s[0], s[1], 1000 + 17 * k) for k, s in enumerate(SIZES)}
    out["smooth"] = smooth_image()
    return out


ENERGY = F(1.75)


def _sphere(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def _from_uv(u, v):
    """unit directions whose (u, v) is close to the one given (float64 trigonometry, rounded)"""
    phi, theta = (np.asarray(u, np.float64) - 0.5) * 2 * np.pi, np.asarray(v, np.float64) * np.pi
    return np.stack([np.sin(phi) * np.sin(theta), np.cos(theta), np.cos(phi) * np.sin(theta)], axis=1).astype(F)


def directions():
    """[N, 3] float32 and the index ranges of the groups: sphere, poles, seam, edges (texel centres and edges of the 64x32 image),
    outside (dir.y beyond [-1, 1]).  Made once for the recording; the tests read them from the fixture, not from here."""
    den = np.float32(1.4e-45)
    one_dn, one_up = np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))
    groups = {}
    groups["sphere"] = _sphere(2048, 7)
    small = np.array([0.0, -0.0, den, -den, 1e-30, -1e-30, 1e-8, -1e-8], F)
    poles = []
    for y in (F(1), -F(1), one_dn, -one_dn):
        for k in range(16):
            poles.append((small[k % 8], y, small[(k // 2 + 3) % 8]))
    groups["poles"] = np.array(poles, F)
    rng = np.random.default_rng(11)
    xs = np.array([0.0, -0.0, den, -den], F)
    seam = np.zeros((128, 3), F)
    seam[:, 0] = xs[np.arange(128) % 4]
    seam[:, 1] = rng.uniform(-0.95, 0.95, 128).astype(F)
    seam[:, 2] = -np.sqrt(1 - seam[:, 1].astype(np.float64) ** 2).astype(F)
    groups["seam"] = seam
    k = np.arange(32)
    u = np.concatenate([(k * 2 + 1) / 64.0, (k * 2 + 0.5) / 64.0])          # edges and centres of columns
    v = np.concatenate([(k + 0.5) / 32.0, (k % 31 + 1) / 32.0])              # centres and edges of rows
    base = _from_uv(u, v)
    nudged = base.copy()
    nudged[:, 0] = np.nextafter(nudged[:, 0], F(np.inf))
    nudged[:, 1] = np.nextafter(nudged[:, 1], F(-np.inf))
    groups["edges"] = np.concatenate([base, nudged])
    out = []
    for y in (one_up, -one_up, F(1.0001), -F(1.0001), F(1.5), -F(1.5), F(3.0e38), -F(3.0e38)):
        for x, z in ((0.0, 0.0), (1e-3, -2e-3), (-0.25, 0.5), (den, -den)):
            out.append((x, y, z))
    groups["outside"] = np.array(out, F)
    ranges, at = {}, 0
    for name, g in groups.items():
        ranges[name] = (at, at + g.shape[0])
        at += g.shape[0]
    return np.concatenate(list(groups.values())).astype(F), ranges
