"""Next-event estimation with one light per record, without a device: the numpy restatement (messyerraytracer_amd/nee.py, what the GPU
tests hold the kernels to byte for byte) and the plans of the casts (csrc/host/record_policy_test.cpp; their host side: tests/test_source_cast_cpu.py).  Fixed inputs, so
every check is deterministic.

The two statistical checks state their bound before they look: 5 standard deviations of the exact distribution, which a correct
estimator misses with probability 6e-7 per comparison.  The unbiased-estimator check runs F = 4096 frames (the first value tried; it
holds there) on 256 hand-made rows x 3 channels; the uniform-selection check counts 65 536 pixels."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import hemisphere as H
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import nee
from messyerraytracer_amd import path as P
from messyerraytracer_amd import shadow as Sh
from messyerraytracer_amd import types as T

F = np.float32
FRAMES = 4096   # F of the unbiased-estimator check


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def hand_made(side=16, seed=2700):
    """side x side surfaces on a tilted, bumpy sheet under five lights of all three kinds: rows, positions, incoming directions."""
    rng = np.random.default_rng(seed)
    n = side * side
    gx, gz = np.meshgrid(np.linspace(-3, 3, side), np.linspace(-3, 3, side))
    p = np.stack([gx.ravel(), 0.2 * np.sin(gx.ravel() * 1.3) + 0.1 * gz.ravel(), gz.ravel()], axis=1).astype(F)
    nrm = np.stack([0.3 * rng.normal(size=n), np.ones(n), 0.3 * rng.normal(size=n)], axis=1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    eye = np.array([0.0, 4.0, 6.0])
    d = p.astype(np.float64) - eye
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    rows = np.zeros(n, T.SURFACE64)
    rows["normal"] = nrm
    rows["n_dot_v"] = np.maximum(-(nrm * d).sum(axis=1), 0.001).astype(F)
    rows["albedo"] = rng.uniform(0.1, 0.9, (n, 3))
    rows["metallic"] = rng.choice([0.0, 0.3, 1.0], n)
    rows["roughness"] = rng.uniform(0.1, 1.0, n)
    rows["specular"] = 0.5
    rows["emission"] = rng.uniform(0, 0.2, (n, 3))
    return rows, p, d


def five_lights():
    ls = np.zeros(5, T.SHADE_LIGHT)
    ls["cast_shadows"], ls["range"], ls["attenuation"], ls["spot_angle"], ls["spot_angle_attenuation"] = 1, 12, 1, 0.7, 1
    ls["type"] = (T.LIGHT_DIRECTIONAL, T.LIGHT_POINT, T.LIGHT_SPOT, T.LIGHT_POINT, T.LIGHT_SPOT)
    ls["direction"] = ((0.3, 1.0, 0.2), (0, 1, 0), (0, 1, 0), (0, 1, 0), (-0.5, 0.8, 0.3))
    ls["position"] = ((0, 0, 0), (1.0, 3.0, 1.0), (0.0, 4.0, 0.0), (-2.5, 0.8, -2.0), (-2.0, 3.0, 1.0))
    ls["color"] = ((1.0, 0.9, 0.8), (2.0, 2.5, 1.0), (3.0, 3.0, 3.5), (0.5, 4.0, 0.7), (2.0, 1.0, 3.0))
    ls["range"][3], ls["attenuation"][3] = 3.0, 2     # a short range: beyond it for most of the sheet
    ls["spot_angle"][4], ls["spot_angle_attenuation"][4] = 0.5, 0.5
    return ls


def test_exports_and_sizes():
    L = capi.load()
    for s in ("mrt_cast_selected_shadows", "mrt_cast_grid_selected_shadows", "mrt_light_selected_surfaces", "mrt_light_grid_selected_surfaces"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert L.mrt_struct_size(capi.STRUCT_LIGHT_SELECT) == C.sizeof(capi.LightSelect) == T.LIGHT_SELECT.itemsize == 24
    assert L.mrt_struct_size(33) == 0 and L.mrt_struct_size(35) == 0
    assert L.mrt_struct_size(capi.STRUCT_SVGF_PARAMS) == 48   # the struct before it is as it was
    assert T.path_select_draw(0) == 256 and T.path_select_draw(32) == 288 and T.LIGHT_NONE == 0xFF
    P_ = C.c_void_p(16)  # never dereferenced: a null context fails first
    d = capi.LightSelect(0, 256, None, 16)
    o = capi.LightOut(16)
    assert L.mrt_cast_selected_shadows(None, P_, P_, 4, C.byref(d), P_, 1, P_, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    assert L.mrt_light_selected_surfaces(None, P_, P_, P_, 4, P_, 1, P_, None, None, C.byref(o), 0) == capi.ERR_INVALID
    cam = capi.camera_look((0, 0, 3), (0, 0, -1), 4, 4, 60.0)
    assert L.mrt_cast_grid_selected_shadows(None, C.byref(cam), 4, 4, 0, 4, P_, C.byref(d), P_, 1, P_, 0xFFFFFFFF, 0) == capi.ERR_INVALID
    assert L.mrt_light_grid_selected_surfaces(None, C.byref(cam), 4, 4, 0, 4, P_, P_, P_, 1, P_, None, None, C.byref(o), 0) == capi.ERR_INVALID


@pytest.mark.parametrize("b", [0, 1, 32])
def test_the_jump_reaches_the_stepped_draw(b):
    """select_lights goes to draw 256 + b through the jump constants; stepping the generator draw by draw gives the same word."""
    pixel = np.concatenate([np.arange(4096, dtype=np.uint64), np.array([2 ** 21 - 1, 2 ** 32 - 1, 1920 * 1080 - 1], np.uint64)])
    hit = np.ones(pixel.shape[0], bool)
    for frame in (0, 3, T.PATH_MAX_FRAME):
        stepped = H.draws(P.stream_seed(pixel, frame), T.path_select_draw(b) + 1)[:, -1]
        for n in (1, 3, 5, 16):
            got = nee.select_lights(pixel, frame, T.path_select_draw(b), n, hit)
            np.testing.assert_array_equal(got, (stepped % np.uint32(n)).astype(np.uint8))
    # not selected: a miss, or a select byte of 0
    sel = (np.arange(pixel.shape[0]) % 3 != 0).astype(np.uint8)
    hit[5::7] = False
    got = nee.select_lights(pixel, 3, T.path_select_draw(b), 5, hit, sel)
    off = ~hit | (sel == 0)
    assert (got[off] == T.LIGHT_NONE).all() and (got[~off] < 5).all()
    np.testing.assert_array_equal(got[~off], nee.select_lights(pixel, 3, T.path_select_draw(b), 5, np.ones_like(hit))[~off])


def test_one_light_is_the_all_lights_path():
    """n_lights == 1: the selected ray is shadow_rays' ray and selected_direct is direct_light, word for word, for each kind of light."""
    rows, p, d = hand_made()
    n = rows.shape[0]
    hit = np.arange(n) % 11 != 3
    pixel = np.arange(n, dtype=np.uint64)
    mask = (np.arange(n) % 5 != 0).astype(np.uint8)
    for l in range(5):
        one = five_lights()[l:l + 1]
        if l == 1:
            one["cast_shadows"] = 0
        light = nee.select_lights(pixel, 7, T.path_select_draw(1), 1, hit)
        assert (light[hit] == 0).all() and (light[~hit] == T.LIGHT_NONE).all()
        rays, traced = nee.selected_shadow_rays(p, rows["normal"], hit, Lg.shadow_lights(one), light)
        want_rays, want_traced = Sh.shadow_rays(p, rows["normal"], hit, Lg.shadow_lights(one))
        np.testing.assert_array_equal(words(rays), words(want_rays))
        np.testing.assert_array_equal(traced, want_traced)
        for m in (None, mask):
            got = nee.selected_direct(rows, p, d, one, light, m, hit=hit)
            want, _ = Lg.direct_light(rows[hit], p[hit], d[hit], one, None if m is None else m[None, hit])
            np.testing.assert_array_equal(words(got[hit, :3]), words(want))
            assert (got[hit, 3] == 1).all() and (got[~hit] == 0).all()
            full = Lg.shade_linear(rows, hit, p, d, one, None if m is None else m[None, :], Lg_env())[0]
            np.testing.assert_array_equal(words(nee.selected_direct(rows, p, d, one, light, m, Lg_env(), hit)), words(full))


def Lg_env():
    env = np.zeros(1, T.ENVIRONMENT)
    env["sky_zenith"], env["sky_horizon"], env["sky_ground"] = (0.15, 0.25, 0.55), (0.6, 0.7, 0.85), (0.15, 0.12, 0.1)
    env["ambient"], env["ambient_energy"] = (1.0, 0.9, 0.8), 0.15
    return env[0]


def test_selected_rays_and_skips():
    """Five lights: every record's ray is the pair's ray of shadow_rays; a light byte of NONE or past the list, a mask byte of 0 and a
    light the all-lights loop skips all give 0 before the environment."""
    rows, p, d = hand_made()
    n = rows.shape[0]
    ls = five_lights()
    ls["cast_shadows"][3] = 0
    hit = np.arange(n) % 13 != 2
    light = nee.select_lights(np.arange(n, dtype=np.uint64), 11, 256, 5, hit)
    assert set(np.unique(light)) == {0, 1, 2, 3, 4, T.LIGHT_NONE}
    rays, traced = nee.selected_shadow_rays(p, rows["normal"], hit, Lg.shadow_lights(ls), light)
    all_rays, all_traced = Sh.shadow_rays(p, rows["normal"], hit, Lg.shadow_lights(ls))
    for i in range(n):
        k = int(light[i])
        if k == T.LIGHT_NONE:
            assert not traced[i] and words(rays[i:i + 1]).tolist() == words(Sh.PLACEHOLDER).tolist()
        else:
            assert traced[i] == all_traced[k * n + i] and words(rays[i:i + 1]).tolist() == words(all_rays[k * n + i:k * n + i + 1]).tolist()
    assert not traced[light == 3].any()   # cast_shadows == 0
    byte = light.copy()
    byte[::9] = 5          # past the list
    mask = (np.arange(n) % 4 != 1).astype(np.uint8)
    got = nee.selected_direct(rows, p, d, ls, byte, mask)
    v = Lg.view_dir(d)
    skipped = 0
    for k in range(5):
        c, active, _, _ = Lg.light_term(rows, p, v, ls[k])
        mine = byte == k
        on = mine & active & (mask != 0)
        np.testing.assert_array_equal(words(got[on, :3]), words((F(0) + c[on]) * F(5)))
        assert (got[mine & ~on, :3] == 0).all() and on.any()
        skipped += int((mine & ~active).sum())
    assert skipped > 0   # the short point light and the spots skip part of the sheet
    assert (got[byte >= 5, :3] == 0).all() and (got[:, 3] == 1).all()


def test_the_estimator_is_unbiased():
    """The mean of selected_direct over FRAMES frames against the all-lights sum, per pixel and channel, within 5 s / sqrt(FRAMES) with
    s the exact standard deviation of the estimator: s^2 = N sum(term_k^2) - (sum term_k)^2 (the estimator is N term_k with probability
    1 / N each)."""
    rows, p, d = hand_made()
    n, ls = rows.shape[0], five_lights()
    N = ls.shape[0]
    v = Lg.view_dir(d)
    terms = np.stack([Lg.light_term(rows, p, v, ls[k])[0].astype(np.float64) for k in range(N)])     # [N, n, 3], 0 where skipped
    total = terms.sum(axis=0)
    s = np.sqrt(np.maximum(N * (terms ** 2).sum(axis=0) - total ** 2, 0.0))
    assert (s > 0).any() and (total > 0).any()
    pixel = np.arange(n, dtype=np.uint64)
    light = np.concatenate([nee.select_lights(pixel, f, T.path_select_draw(0), N, np.ones(n, bool)) for f in range(FRAMES)])
    est = nee.selected_direct(np.tile(rows, FRAMES), np.tile(p, (FRAMES, 1)), np.tile(d, (FRAMES, 1)), ls, light)
    mean = est[:, :3].astype(np.float64).reshape(FRAMES, n, 3).mean(axis=0)
    bound = 5.0 * s / np.sqrt(FRAMES)
    worst = np.abs(mean - total) / np.where(bound > 0, bound, 1.0)
    print("largest |mean - sum| over its bound: %.3f" % worst.max())
    assert (np.abs(mean - total) <= bound).all(), float(worst.max())
    # the all-lights sum of the restatement is that total, up to its float32 additions
    ref, _ = Lg.direct_light(rows, p, d, ls)
    np.testing.assert_allclose(ref, total, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("n_lights", [3, 5, 16])
def test_the_selection_is_uniform(n_lights):
    """65 536 pixels: the count of every light within 5 standard deviations of the binomial distribution B(n, 1 / N)."""
    n = 65536
    light = nee.select_lights(np.arange(n, dtype=np.uint64), 0, T.path_select_draw(0), n_lights, np.ones(n, bool))
    counts = np.bincount(light, minlength=n_lights)
    assert counts.shape[0] == n_lights and counts.sum() == n
    q = 1.0 / n_lights
    sigma = np.sqrt(n * q * (1 - q))
    print("counts - n / N over sigma:", np.round((counts - n * q) / sigma, 2))
    assert (np.abs(counts - n * q) <= 5 * sigma).all()


def test_selected_shadow_policy_driver():
    exe = mbuild.build_record_policy_test()
    r = subprocess.run([exe, "selected_shadow"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
