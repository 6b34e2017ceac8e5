"""The renderer's channels and its 8-bit image without a device: the library exports the four entry points, the struct size and layout
agree and the calls reject a null context; the host-side refusals and the selection mask (csrc/host/channel_data_test.cpp); the numpy
restatement (messyerraytracer_amd/channels.py, what the GPU tests hold the kernels to byte for byte) against values recorded from the
reference's own shade_normal .. shade_barycentric (shade_pass.h:337-395), shade_albedo .. shade_fresnel (:732-884) and
RayImage::to_image (ray_image.cpp:22-35) in tests/golden/channels_reference.npz.  Only floorf, sqrtf and fp32 arithmetic
enter, so every tuple is compared bit for bit: no tolerance, no tuple left out.  The 8 tuples of kind 8 were given a NaN on purpose (a
NaN or infinite vertex UV, a NaN barycentric, position or t); where the recording holds a NaN the restatement must hold one too:
N_NAN_TUPLES below is their count, and no other tuple's recording holds a NaN."""
import ctypes as C
import os
import subprocess

import numpy as np

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import channels as Ch
from messyerraytracer_amd import path as P
from messyerraytracer_amd import surface as S
from messyerraytracer_amd import texture as X
from messyerraytracer_amd import types as T

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "channels_reference.npz")
N_IMAGES = 4
N_NAN_TUPLES = 8
HAS_N, HAS_ID, HAS_UV, HAS_T, PRIM_OK, ID_OK, FREE_PRIM, MISS = (1 << k for k in range(8))

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        g = np.load(GOLDEN)
        g = {k: g[k] for k in g.files}
        g["images"] = [g[f"image_{k}"] for k in range(N_IMAGES)]
        _FIXTURE.append(g)
    return _FIXTURE[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_exports_sizes_and_layouts():
    L = capi.load()
    for s in ("mrt_shade_channels", "mrt_shade_grid_channels", "mrt_finish_color", "mrt_image_to_rgba8"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert capi.STRUCT_CHANNEL_OUT == 24
    assert L.mrt_struct_size(capi.STRUCT_CHANNEL_OUT) == C.sizeof(capi.ChannelOut) == 192
    assert L.mrt_struct_size(23) == 0 and L.mrt_struct_size(25) == 0
    assert [getattr(capi.ChannelOut, n).offset for n, _ in capi.ChannelOut._fields_] == [0, 4, 8, 12, 16, 104]
    names = ("COLOR", "NORMAL", "DEPTH", "BARYCENTRIC", "POSITION", "PRIM_ID", "HIT_MASK", "ALBEDO", "WIREFRAME", "UV", "FRESNEL", "COUNT")
    assert [getattr(capi, "CHANNEL_" + n) for n in names] == list(range(12)) == [getattr(Ch, n) for n in names]
    assert L.mrt_version() == 1
    # the structs before it are as they were
    assert L.mrt_struct_size(capi.STRUCT_PANORAMA) == C.sizeof(capi.Panorama) and L.mrt_struct_size(capi.STRUCT_SURFACE_OUT) == C.sizeof(capi.SurfaceOut)


def test_null_context_is_invalid():
    """(With a context, every bad descriptor is refused before any device work: test_channels_gpu.py.)"""
    L = capi.load()
    d = capi.channel_out(0.25, 1.0, rgba={capi.CHANNEL_DEPTH: 16})
    cam = capi.Camera()
    assert L.mrt_shade_channels(None, 16, 16, 4, C.byref(d), 0) == capi.ERR_INVALID
    assert L.mrt_shade_channels(None, None, None, 0, None, 0) == capi.ERR_INVALID
    assert L.mrt_shade_grid_channels(None, C.byref(cam), 4, 4, 0, 4, 16, C.byref(d), 0) == capi.ERR_INVALID
    assert L.mrt_finish_color(None, 16, 4, 0, 16, 16, 0) == capi.ERR_INVALID
    assert L.mrt_image_to_rgba8(None, 16, 4, 16, 0) == capi.ERR_INVALID


def test_channel_data_driver():
    exe = mbuild.build_channel_data_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


def _groups(g):
    """The channel tuples as batches shade_channels takes: one batch per set of resident arrays and pair of ranges.  As recorded, tuple i
    of all N is triangle i with its own material i and binding i (the prim id enters PRIM_ID's hash); a prim out of range is N + i, an
    id out of range N + i; a free prim id (no array resident) is the tuple's own word."""
    cin = g["c_in"]
    words = cin.view(np.uint32)
    fl = words[:, 8]
    N = cin.shape[0]
    every = np.arange(N)
    mats = np.zeros(N, T.MATERIAL)
    mats["albedo"], mats["roughness"], mats["specular"] = cin[:, 36:39], 0.5, 0.5
    ids = np.where((fl & ID_OK) != 0, every, N + every).astype(np.uint32)
    b = np.zeros(N, T.MATERIAL_TEXTURES)
    b["albedo_texture"], b["normal_texture"], b["normal_scale"] = words[:, 43], words[:, 44], cin[:, 45]
    key = np.stack([fl & 15, words[:, 47], words[:, 48]], axis=1)
    for k in np.unique(key, axis=0):
        idx = np.nonzero((key == k).all(axis=1))[0]
        e, w, f = cin[idx], words[idx], fl[idx]
        present = int(k[0])
        prim = np.where((f & PRIM_OK) != 0, idx, N + idx).astype(np.uint32)
        prim = np.where((f & FREE_PRIM) != 0, w[:, 46], prim).astype(np.uint32)
        assert present == 0 or not (f & FREE_PRIM).any()
        shade = S.ShadeData(N, mats, ids if present & HAS_ID else None, cin[:, 9:18].reshape(N, 3, 3) if present & HAS_N else None,
                            cin[:, 18:24].reshape(N, 3, 2) if present & HAS_UV else None)
        if (f & FREE_PRIM).any():
            shade = None                                                                   # (recorded against an empty SceneShadeData)
        tex = X.TextureSet(g["images"], b, cin[:, 24:36] if present & HAS_T else None)
        yield idx, e, (f & MISS) == 0, prim, shade, tex, e[0, 47], e[0, 48]


def _restated(g):
    out = np.zeros(g["c_out"].shape, F)
    for idx, e, hit, prim, shade, tex, inv_d, inv_p in _groups(g):
        got = Ch.shade_channels(e[:, 0:3], e[:, 40:43], e[:, 3:6], hit, e[:, 39], prim, e[:, 6], e[:, 7], inv_d, inv_p, shade, tex)
        for c in Ch.ALL:
            out[idx, c - 1] = got[c]
    return out


def test_fixture_covers_what_it_must():
    g = fixture()
    cin, words, out = g["c_in"], g["c_in"].view(np.uint32), g["c_out"]
    kind, fl, u, v = words[:, 49], words[:, 8], cin[:, 6], cin[:, 7]
    w = (F(1) - u) - v
    for k, least in ((0, 1900), (1, 64), (2, 130), (3, 40), (4, 48), (5, 260), (6, 96), (7, 32), (8, N_NAN_TUPLES)):
        assert (kind == k).sum() >= least, k
    # barycentrics: w at 0 and on either side of it; u, v or both 0
    b = kind == 1
    assert (w[b] == 0).any() and (w[b] > 0).any() and (w[b] < 0).any() and (np.abs(w[b][w[b] != 0]).min() < 1e-7)
    assert (b & (u == 0) & (v != 0)).any() and (b & (v == 0) & (u != 0)).any() and (b & (u == 0) & (v == 0)).any()
    # wireframe: the minimum, each of the three in turn, at 0.01f and 0.03f exactly and one ulp to either side
    m = np.minimum(np.minimum(w, u), v)
    for mark in (F(0.01), F(0.03)):
        for x in (mark, np.nextafter(mark, F(1)), np.nextafter(mark, F(0))):
            for a in (w, u, v):
                assert ((kind == 2) & (m == x) & (a == x)).any(), (mark, x)
    s = (m[kind == 2] - F(0.01)) / (F(0.03) - F(0.01))
    assert (s < 0).sum() >= 10 and ((s > 0) & (s < 1)).sum() >= 10 and (s > 1).sum() >= 10
    # depth: both clamps, the inside, exactly 0 and exactly 1
    x = F(1) - cin[:, 39] * cin[:, 47]
    d = kind == 3
    assert (x[d] < 0).any() and (x[d] > 1).any() and ((x[d] > 0) & (x[d] < 1)).any() and (x[d] == 0).any() and (x[d] == 1).any()
    # position: negative coordinates, exact multiples of the range, tiny negatives whose fraction rounds to 1
    p = cin[kind == 4][:, 40:43] * cin[kind == 4][:, 48:49]
    fr = (p - np.floor(p)).astype(F)
    assert (p < 0).any() and ((p == np.floor(p)) & (p != 0)).any() and ((p < 0) & (fr == 1)).sum() >= 8
    # prim ids
    ids = words[kind == 5][:, 46]
    for x in (0, 1, 2 ** 31, 0xFFFFFFFE):
        assert (ids == x).any()
    assert np.unique(ids).shape[0] >= 256
    # fresnel: q below 0, above 1, inside -- taken from the recording's own blue channel (0.3 + q * 0.7)
    q = out[kind == 6][:, Ch.FRESNEL - 1, 0]
    assert (q == 0).sum() >= 16 and (q == 1).sum() >= 16 and ((q > 0) & (q < 1)).sum() >= 16
    # shade data: every combination of resident arrays, ids out of range, textures bound and not
    gen = kind == 0
    for present in range(16):
        mk = gen & ((fl & 15) == present)
        assert mk.sum() >= 100 and (mk & ((fl & PRIM_OK) == 0)).sum() >= 10 and (mk & ((fl & ID_OK) == 0)).sum() >= 10
        for at in (False, True):
            for nt in (False, True):
                assert (mk & ((words[:, 43] != X.NO_TEXTURE) == at) & ((words[:, 44] != X.NO_TEXTURE) == nt)).sum() >= 20
    assert ((fl & MISS) != 0).sum() >= 32
    # to_rgba8's values
    bi = g["b_in"]
    for k in range(256):
        h = (F(k) + F(0.5)) / F(255)
        for x in (F(k) / F(255), h, np.nextafter(h, F(2)), np.nextafter(h, F(-1))):
            assert (bits(bi) == bits(x)).any(), k
    assert (bits(bi) == bits(F(-0.0))).any() and (bi == np.inf).any() and (bi == -np.inf).any() and np.isnan(bi).sum() >= 2
    assert (bi < 0).sum() >= 50 and (bi > 1).sum() >= 50
    # the NaNs are where they were put, and nowhere else
    nan_rows = np.isnan(out).any(axis=(1, 2))
    assert nan_rows.sum() == N_NAN_TUPLES and (kind[nan_rows] == 8).all()


def test_channels_equal_the_reference_bit_for_bit():
    g = fixture()
    got, want = _restated(g), g["c_out"]
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all()                                                        # NaN in both
    assert np.isnan(want).any(axis=(1, 2)).sum() == N_NAN_TUPLES
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])
    # the textures and the smooth normals did something
    kind = g["c_in"].view(np.uint32)[:, 49]
    plain = np.zeros(want.shape, F)
    for idx, e, hit, prim, shade, tex, inv_d, inv_p in _groups(g):
        p = Ch.shade_channels(e[:, 0:3], e[:, 40:43], e[:, 3:6], hit, e[:, 39], prim, e[:, 6], e[:, 7], inv_d, inv_p, shade, None, (Ch.NORMAL, Ch.ALBEDO))
        plain[idx, Ch.NORMAL - 1], plain[idx, Ch.ALBEDO - 1] = p[Ch.NORMAL], p[Ch.ALBEDO]
    for c in (Ch.NORMAL, Ch.ALBEDO):
        assert ((bits(plain[:, c - 1]) != bits(want[:, c - 1])).any(axis=1) & (kind == 0)).sum() >= 60, c
    # a miss is {0, 0, 0, 1} in every channel
    miss = (g["c_in"].view(np.uint32)[:, 8] & MISS) != 0
    assert (want[miss] == F([0, 0, 0, 1])).all()


def test_to_rgba8_equals_the_reference_bit_for_bit():
    g = fixture()
    np.testing.assert_array_equal(Ch.to_rgba8(g["b_in"]), g["b_out"])
    np.testing.assert_array_equal(Ch.to_rgba8(g["c_out"]), g["c_out8"])                    # the channels' own bytes, NaNs included
    np.testing.assert_array_equal(Ch.to_rgba8(_restated(g)), g["c_out8"])
    np.testing.assert_array_equal(Ch.to_rgba8(F([0, 1, 0.5, np.nan, -np.inf, np.inf, -0.0])), np.uint8([0, 255, 128, 0, 0, 255, 0]))


def test_finish_color_is_the_path_finish_on_hits_and_identity_on_misses():
    rng = np.random.default_rng(5)
    n = 4096
    lit = np.zeros((n, 4), F)
    lit[:, :3] = rng.uniform(0, 4, (n, 3)).astype(F) * rng.choice(F([0, 1e-3, 1, 8]), (n, 1))
    lit[:, 3] = rng.integers(0, 2, n)
    hit = lit[:, 3] != 0
    assert hit.sum() > 1000 and (~hit).sum() > 1000
    state = P.init_state(n)
    state["radiance"] = lit[:, :3]
    for mode in range(5):
        got, want = Ch.finish_color(lit, mode), P.path_finish(state, mode)
        np.testing.assert_array_equal(bits(got[hit]), bits(want[hit]))
        np.testing.assert_array_equal(bits(got[~hit, :3]), bits(lit[~hit, :3]))
        assert (got[:, 3] == 1).all()
        assert mode == 0 or (bits(got[hit, :3]) != bits(lit[hit, :3])).any()
