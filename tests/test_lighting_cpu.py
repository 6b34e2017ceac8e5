"""Direct light on resolved surfaces without a device: the library exports the three entry points and the calls reject a null context
and bad arguments before any device work; the host-side checks, the kernel's copy of a light list and pow01
(csrc/host/light_data_test.cpp); pow01's sweep against numpy's float64 power; the numpy restatement (messyerraytracer_amd/lighting.py,
what the GPU tests hold the kernel to byte for byte) against values recorded from the reference's own distribution_ggx,
fresnel_schlick, geometry_smith_ggx, compute_distance_attenuation, compute_spot_attenuation, cook_torrance_multi_light and sky_color
(tests/golden/lighting_reference.npz): bit for bit wherever neither pow nor cos is involved, and elsewhere within twice
the largest difference measured (pow01 against the host's powf), which is printed and asserted.

Measured on the fixture: on the 1423 point and spot tuples away from the attenuation skip the largest relative difference
in a channel is 0 (pow01 returned the host powf's bits in every one), so twice that holds them bit for bit; on the 1024 recorded calls of
the two attenuation helpers alone it is 6.671e-08 (one float ulp of a result near 1), asserted as 1.3343e-07."""
import ctypes as C
import os
import subprocess

import numpy as np

from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import types as T

P = C.c_void_p(16)  # a pointer no call may dereference: every case below fails its checks first
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lighting_reference.npz")
# §4.12's rule: a bound is twice the largest difference measured (the module's docstring has the measurements).
TUPLE_BOUND = 2 * 0.0
HELPER_BOUND = 1.3343e-07   # 2 x 6.671e-08
E6 = F(1e-6)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_exports_sizes_and_layouts():
    L = capi.load()
    for s in ("mrt_shadow_lights", "mrt_light_surfaces", "mrt_light_grid_surfaces"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert L.mrt_struct_size(capi.STRUCT_SHADE_LIGHT) == T.SHADE_LIGHT.itemsize == 64
    assert L.mrt_struct_size(capi.STRUCT_ENVIRONMENT) == T.ENVIRONMENT.itemsize == 64
    assert L.mrt_struct_size(capi.STRUCT_LIGHT_OUT) == C.sizeof(capi.LightOut) == 8
    assert (capi.STRUCT_SHADE_LIGHT, capi.STRUCT_ENVIRONMENT, capi.STRUCT_LIGHT_OUT) == (11, 12, 13)
    assert L.mrt_struct_size(10) == 0 and L.mrt_struct_size(14) == 0
    # the first 32 bytes of a shade light are mrt_light field for field
    for n in T.LIGHT.names:
        assert T.SHADE_LIGHT.fields[n][1] == T.LIGHT.fields[n][1] and T.SHADE_LIGHT.fields[n][0] == T.LIGHT.fields[n][0]
    assert [T.SHADE_LIGHT.fields[n][1] for n in T.SHADE_LIGHT.names] == [0, 4, 8, 20, 32, 44, 48, 52, 56, 60]
    assert [T.ENVIRONMENT.fields[n][1] for n in T.ENVIRONMENT.names] == [0, 12, 24, 36, 48, 52]


def lights3():
    ls = np.zeros(3, T.SHADE_LIGHT)
    ls["type"], ls["cast_shadows"], ls["range"], ls["attenuation"], ls["spot_angle"], ls["spot_angle_attenuation"] = (0, 1, 2), (1, 0, 1), 10, 1, 0.7, 1
    ls["position"], ls["direction"], ls["color"] = ((1, 2, 3), (4, 5, 6), (7, 8, 9)), (0, -1, 0), (1, 0.5, 0.25)
    return ls


def test_shadow_lights_copies_the_shadow_half():
    ls = lights3()
    got = capi.shadow_lights(ls)
    assert got.dtype == T.LIGHT and got.shape == (3,)
    np.testing.assert_array_equal(got.view(np.uint8).reshape(3, 32), ls.view(np.uint8).reshape(3, 64)[:, :32])
    np.testing.assert_array_equal(got.view(np.uint8), Lg.shadow_lights(ls).view(np.uint8))
    assert capi.shadow_lights(ls[:0]).shape == (0,)
    L = capi.load()
    assert L.mrt_shadow_lights(None, 1, P) == capi.ERR_INVALID and L.mrt_shadow_lights(P, 1, None) == capi.ERR_INVALID
    assert L.mrt_shadow_lights(None, 0, None) == 0


def test_null_context_is_invalid():
    """(With a context, every bad argument is checked before any device work: test_lighting_gpu.py.)"""
    L = capi.load()
    out = capi.LightOut(16)
    cam = capi.Camera()
    ls = lights3()
    lp = ls.ctypes.data_as(C.c_void_p)
    for o in (C.byref(out), None):
        for n in (0, 3, 17):
            assert L.mrt_light_surfaces(None, P, P, P, 1, lp, n, None, None, o, 0) == capi.ERR_INVALID
            assert L.mrt_light_surfaces(None, P, P, P, 0, lp, n, None, None, o, 0) == capi.ERR_INVALID
            assert L.mrt_light_grid_surfaces(None, C.byref(cam), 4, 4, 0, 4, P, P, lp, n, None, None, o, 0) == capi.ERR_INVALID
    assert L.mrt_light_surfaces(None, None, None, None, 1, None, 0, None, None, None, 1 << 20) == capi.ERR_INVALID


def test_light_data_driver():
    exe = mbuild.build_light_data_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


# ---- pow01 ----------------------------------------------------------------------------------------------------------------------------

def sweep_bases():
    rng = np.random.default_rng(1)
    small = 2.0 ** -rng.uniform(0, 149, 1 << 16)                      # results that underflow towards 0
    edge = [1 - 2.0 ** -24, 2.0 ** -149, 2.0 ** -126, 2.0 ** -127, 1.0, 0.0, 0.5, 2.0 ** -0.5]
    return np.concatenate([np.arange(65537, dtype=np.float64) / 65536, rng.random(1 << 20), small, edge]).astype(F)


def test_pow01_sweep():
    b = sweep_bases()
    total = differ = worst = 0
    for e in (0.25, 0.5, 1, 2, 3.7, 8, 16):
        got = Lg.pow01(b, F(e))
        with np.errstate(under="ignore"):
            want = np.power(b.astype(np.float64), np.float64(F(e))).astype(F)
        d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        total, differ, worst = total + d.size, differ + int((d > 0).sum()), max(worst, int(d.max()))
        if e == 1:
            np.testing.assert_array_equal(bits(got), bits(b))          # pow01(b, 1) == b for every b
    print(f"pow01 sweep: {differ} of {total} points differ ({differ / total:.2e}), worst {worst} ulp")
    assert worst <= 1


def test_pow01_selects_and_ends():
    assert Lg.pow01(F(0), F(0)) == 1 and Lg.pow01(F(0.3), F(0)) == 1 and Lg.pow01(F(0), F(2)) == 0 and Lg.pow01(F(1), F(3.7)) == 1
    assert Lg.pow01(F(0.25), F(0.5)) == F(0.5) and Lg.pow01(F(0.5), F(149)) == F(2.0 ** -149) and Lg.pow01(F(0.5), F(151)) == 0
    assert Lg.pow01(F(1e-30), F(16)) == 0
    b = np.array([0.1, 0.9], F)
    assert Lg.pow01(b, F(2)).dtype == F and Lg.pow01(b, np.array([1, 0], F)).tolist() == [float(b[0]), 1.0]


# ---- the restatement against the reference's own functions -----------------------------------------------------------------------------

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        g = np.load(GOLDEN)
        g = {k: g[k] for k in g.files}
        n = g["kind"].shape[0]
        rows = np.zeros(n, T.SURFACE64)
        for k in ("normal", "n_dot_v", "albedo", "metallic", "roughness", "specular"):
            rows[k] = g[k]
        g["rows"] = rows
        g["lights"] = g["lights"].view(T.SHADE_LIGHT).reshape(n, 16) if g["lights"].dtype != T.SHADE_LIGHT else g["lights"]
        # every tuple through the restatement once: rgb, and per light the attenuation and the contribution it would have made at atten = 1
        got = np.zeros((n, 3), F)
        atten = np.full((n, 16), np.nan, F)
        full = np.zeros((n, 16, 3), F)
        with np.errstate(all="ignore"):
            for l in range(16):
                for i in np.nonzero(g["n_lights"] > l)[0]:
                    r, p, v = rows[i:i + 1], g["p"][i:i + 1], g["v"][i:i + 1]
                    c, active, powed, a = Lg.light_term(r, p, v, g["lights"][i, l], g["lit"][i:i + 1, l])
                    if active[0]:
                        got[i] = got[i] + c[0]
                    if powed[0]:
                        atten[i, l] = a[0]
                    plain = g["lights"][i, l].copy()
                    plain["attenuation"], plain["spot_angle_attenuation"] = 0, 0          # pow01(., 0) = 1
                    full[i, l] = Lg.light_term(r, p, v, plain, g["lit"][i:i + 1, l])[0][0]
        g["got"], g["got_atten"], g["full"] = got, atten, full
        # tuples with a light whose recorded attenuation lies within 2 ulp of 1e-6f: either side of the skip
        ra = g["atten"]
        du = np.abs(ra.view(np.int32).astype(np.int64) - int(E6.view(np.int32)))
        g["near"] = (np.isfinite(ra) & (du <= 2) & (np.arange(16)[None, :] < g["n_lights"][:, None])).any(axis=1)
        types = np.where(np.arange(16)[None, :] < g["n_lights"][:, None], g["lights"]["type"], 0)
        g["directional_only"] = (types == 0).all(axis=1)
        _FIXTURE.append(g)
    return _FIXTURE[0]


def test_fixture_covers_what_it_must():
    g = fixture()
    kind, n, L0 = g["kind"], g["kind"].shape[0], g["lights"][:, 0]
    assert 1900 <= n <= 2200
    for k, least in ((0, 300), (1, 300), (2, 300), (3, 100), (4, 20), (5, 100), (6, 60), (7, 50), (8, 60), (9, 120), (10, 20), (11, 80), (12, 8)):
        assert (kind == k).sum() >= least, k
    lit = (g["rgb"] != 0).any(axis=1)
    for k in (0, 1, 2, 7, 8, 9, 10, 11):
        assert lit[kind == k].mean() > 0.25, k                                 # the general kinds are not mostly black
    to = L0["position"] - g["p"]
    dist = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2])
    k3 = kind == 3
    assert (dist[k3] == L0["range"][k3]).sum() >= 30 and (dist[k3] < L0["range"][k3]).sum() >= 30 and (dist[k3] > L0["range"][k3]).sum() >= 30
    assert (np.abs(dist[k3].view(np.int32) - L0["range"][k3].view(np.int32)) <= 1).all()
    assert (dist[kind == 4] < E6).all() and (g["rgb"][kind == 4] == 0).all() and (g["rgb"][k3 & (dist > L0["range"])] == 0).all()
    k5 = kind == 5
    co = Lg.cosf(L0["spot_angle"][k5])
    lv = (to[k5] / dist[k5, None]).astype(F)
    d5 = L0["direction"][k5]
    ca = (lv[:, 0] * d5[:, 0] + lv[:, 1] * d5[:, 1]) + lv[:, 2] * d5[:, 2]
    assert (ca == co).sum() >= 30 and (ca == np.nextafter(co, F(2))).sum() >= 30 and (ca == np.nextafter(co, F(-2))).sum() >= 30
    k6 = kind == 6
    ndl = L0["direction"][k6][:, 1]
    assert (g["normal"][k6] == (0, 1, 0)).all() and (ndl == 0).sum() >= 15 and (ndl == F(1.4e-45)).sum() >= 8 and (ndl == F(-1.4e-45)).sum() >= 8
    assert (g["n_dot_v"][kind == 7] == F(0.001)).all()
    k8 = kind == 8
    for ro in (0.04, 1.0):
        for m in (0.0, 1.0):
            assert ((g["roughness"][k8] == F(ro)) & (g["metallic"][k8] == F(m))).sum() >= 15
    for e in (1, 2, 0.5, 0):
        assert (L0["attenuation"][kind == 9] == F(e)).sum() >= 30
    k10 = kind == 10
    assert (L0["direction"][k10] == -g["v"][k10]).all() and lit[k10].all()
    k11 = kind == 11
    assert (g["n_lights"][k11] == 16).all() and (g["n_lights"][~k11] == 1).all()
    L11, lit11 = g["lights"][k11], g["lit"][k11]
    assert (L11["cast_shadows"] == 0).sum() >= 200 and (lit11 == 0).sum() >= 300 and (lit11[L11["cast_shadows"] == 0] == 1).all()
    assert all((L11["type"] == t).sum() >= 300 for t in (0, 1, 2))
    assert np.isfinite(g["rgb"]).all()


def test_helpers_equal_the_reference_bit_for_bit():
    """distribution_ggx, fresnel_schlick, geometry_smith_ggx and sky_color: no pow, no cos"""
    g = fixture()
    a, want = g["fn_in"], g["fn_out"]
    np.testing.assert_array_equal(bits(Lg.distribution_ggx(a[:, 0], a[:, 1])), bits(want[:, 0]))
    np.testing.assert_array_equal(bits(Lg.fresnel_schlick(a[:, 0], a[:, 2])), bits(want[:, 1]))
    np.testing.assert_array_equal(bits(Lg.geometry_smith_ggx(a[:, 0], a[:, 3], a[:, 1])), bits(want[:, 2]))
    env = np.zeros(a.shape[0], T.ENVIRONMENT)
    env["sky_zenith"] = a[:, 0:3]
    env["sky_horizon"] = np.stack([a[:, 3], a[:, 4] * F(0.1), a[:, 5] * F(0.1)], axis=1)
    env["sky_ground"] = np.stack([a[:, 6], a[:, 7], a[:, 1] * a[:, 2]], axis=1)
    d = np.stack([a[:, 3] - F(0.5), (a[:, 0] - F(0.5)) * F(2.5), a[:, 2]], axis=1).astype(F)
    got = np.concatenate([Lg.sky_gradient(d[i:i + 1], env[i]) for i in range(a.shape[0])])
    np.testing.assert_array_equal(bits(got), bits(want[:, 5:8]))
    t = d[:, 1] * F(0.5) + F(0.5)
    assert (t > F(0.5)).sum() > 100 and (t < F(0.5)).sum() > 100 and (t == F(0.5)).sum() >= 16


def rel_diff(got, want):
    with np.errstate(all="ignore"):
        r = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.abs(want.astype(np.float64))
    return np.where(got == want, 0.0, r)


def test_attenuation_helpers_within_the_pow_bound():
    """compute_distance_attenuation and compute_spot_attenuation: exact where the exponent is 0 or 1, else pow01 against powf"""
    g = fixture()
    a, want = g["fn_in"], g["fn_out"]
    got = Lg.distance_attenuation(a[:, 4], a[:, 5], a[:, 6])
    lv = np.stack([a[:, 0], a[:, 3], a[:, 2]], axis=1)               # (the reference was given -L, which it negates again)
    got_s = np.concatenate([Lg.spot_attenuation(lv[i:i + 1], np.array([a[i, 0] * a[i, 1], a[i, 3] * a[i, 1], a[i, 2] * a[i, 1]], F), Lg.cosf(a[i, 7])[0], a[i, 6])[0]
                            for i in range(a.shape[0])])
    exact = (a[:, 6] == 0) | (a[:, 6] == 1)
    np.testing.assert_array_equal(bits(got[exact]), bits(want[exact, 3]))
    np.testing.assert_array_equal(bits(got_s[exact]), bits(want[exact, 4]))
    worst = max(rel_diff(got, want[:, 3]).max(), rel_diff(got_s, want[:, 4]).max())
    print(f"attenuation helpers: largest relative difference {worst:.6e}")
    assert worst <= HELPER_BOUND and (got_s > 0).sum() > 100 and (got > 0).sum() > 500


def test_directional_tuples_equal_the_reference_bit_for_bit():
    g = fixture()
    k = g["directional_only"]
    assert k.sum() >= 500
    np.testing.assert_array_equal(bits(g["got"][k]), bits(g["rgb"][k]))


def test_point_and_spot_tuples_within_the_pow_bound():
    g = fixture()
    k = ~g["directional_only"] & ~g["near"]
    assert k.sum() >= 1100
    r = rel_diff(g["got"][k], g["rgb"][k])
    assert np.isfinite(r).all()                                                  # (a zero on one side only would be infinite)
    exact = (r == 0).all(axis=1)
    print(f"point and spot tuples: {k.sum()} tuples, {exact.sum()} bit for bit, largest relative difference in a channel {r.max():.3e}")
    assert r.max() <= TUPLE_BOUND
    # a tuple whose exponents are all 0 or 1 never differs: pow01(b, 1) == b == powf(b, 1)
    L, nl = g["lights"], g["n_lights"]
    live = np.arange(16)[None, :] < nl[:, None]
    plain = (np.isin(L["attenuation"], (0, 1)) & np.isin(L["spot_angle_attenuation"], (0, 1)) | ~live).all(axis=1)
    assert (k & plain).sum() >= 100 and exact[plain[k]].all()
    # the recorded attenuations themselves
    ra, ga = g["atten"][k], g["got_atten"][k]
    local = live[k] & (L["type"][k] != T.LIGHT_DIRECTIONAL)
    both = np.isfinite(ra) & np.isfinite(ga) & local
    assert ((np.isfinite(ra) & local) == (np.isfinite(ga) & local)).all() and both.sum() >= 1000
    assert rel_diff(ga[both], ra[both]).max() <= TUPLE_BOUND


def test_tuples_at_the_attenuation_skip():
    """Recorded attenuation within 2 ulp of 1e-6f: pow01 and powf may land on either side of `atten < 1e-6f`.  The list is small, and
    on it the difference is at most 1e-6 of what the light contributes at full strength (atten = 1)."""
    g = fixture()
    near = g["near"]
    n = near.shape[0]
    assert 8 <= near.sum() <= n // 100
    assert (g["kind"][near] == 12).all()                                        # only the ones put there on purpose
    diff = np.abs(g["got"][near].astype(np.float64) - g["rgb"][near].astype(np.float64))
    cap = 1e-6 * np.abs(g["full"][near].astype(np.float64)).sum(axis=1)
    straddle = ((g["got"][near] == 0).all(axis=1) != (g["rgb"][near] == 0).all(axis=1)).sum()
    print(f"at the skip: {near.sum()} tuples, {straddle} on different sides, largest difference / cap {np.max(diff / np.maximum(cap, 1e-300)):.3e}")
    assert (np.abs(g["full"][near]).sum(axis=(1, 2)) > 0).all()
    assert (diff <= cap).all()


def test_shade_linear_hand_written_cases():
    """The three terms around the direct light, and a miss, from the text of shade_material (shade_pass.h:669-716)."""
    rows = np.zeros(3, T.SURFACE64)
    rows["normal"], rows["n_dot_v"], rows["albedo"], rows["metallic"] = ((0, 1, 0), (0, -1, 0), (0, 0, 0)), 1, ((0.5, 0.25, 1.0),) * 3, (0, 0.5, 0)
    rows["roughness"], rows["specular"], rows["emission"] = 0.5, 0.5, ((0, 0, 0), (1, 2, 3), (0, 0, 0))
    hit = np.array([True, True, False])
    d = np.array([[0, -1, 0], [0, 1, 0], [0.3, 0.5, 0.1]], F)
    p = np.zeros((3, 3), F)
    env = np.zeros(1, T.ENVIRONMENT)[0]
    env["sky_zenith"], env["sky_horizon"], env["sky_ground"], env["ambient"], env["ambient_energy"] = (0.25, 0.5, 1), (0.5, 0.5, 0.5), (0.125, 0, 0.25), (1, 0.5, 2), 0.5
    none = np.zeros(0, T.SHADE_LIGHT)
    out, n_pow = Lg.shade_linear(rows, hit, p, d, none, None, None)
    assert n_pow == 0 and out.dtype == F
    np.testing.assert_array_equal(out, np.array([[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0]], F))
    out, _ = Lg.shade_linear(rows, hit, p, d, none, None, env)
    # up-facing: blend 1 -> the zenith colour; diff = albedo: ((0.5*0.25)*1)*0.5, ((0.25*0.5)*0.5)*0.5, ((1*1)*2)*0.5
    np.testing.assert_array_equal(out[0], np.array([0.0625, 0.03125, 1.0, 1], F))
    # down-facing: blend 0 -> the ground colour; diff = albedo * 0.5; plus the emission
    np.testing.assert_array_equal(out[1], np.array([((0.25 * 0.125) * 1) * 0.5 + 1, 0 + 2, ((0.5 * 0.25) * 2) * 0.5 + 3, 1], F))
    # a miss: t = 0.5 * 0.5 + 0.5 = 0.75 -> horizon + (zenith - horizon) * 0.5; alpha 0
    np.testing.assert_array_equal(out[2], np.array([0.375, 0.5, 0.75, 0], F))
    down = Lg.sky_gradient(np.array([[0, -0.5, 0], [0, 0, 0]], F), env)      # t = 0.25 -> ground + (horizon - ground) * 0.5; t = 0.5: the lower branch
    np.testing.assert_array_equal(down, np.array([[0.3125, 0.25, 0.375], [0.5, 0.5, 0.5]], F))
    # one directional light straight down the normal of row 0, by hand from the text: v = n = L = h
    sun = np.zeros(1, T.SHADE_LIGHT)
    sun["direction"], sun["color"] = (0, 1, 0), (2, 2, 2)
    got, _ = Lg.shade_linear(rows[:1], hit[:1], p[:1], d[:1], sun, None, None)
    a2 = F(0.0625)
    D = a2 / ((Lg.PI * a2) * a2 + F(1e-7))                                    # den = 1 * (a2 - 1) + 1 = a2
    g1 = F(2) / ((F(1) + np.sqrt(a2 + (F(1) - a2))) + F(1e-7))
    f0 = (F(0.04) * F(0.5)) * F(2)                                            # t = 0: F = f0
    spec = (D * (g1 * g1)) / (F(4) + F(1e-7))
    want = [(((F(alb) * (F(1) - f0)) * Lg.DIFF_SCALE + f0 * spec) * F(2)) * F(1) for alb in (0.5, 0.25, 1.0)] + [F(1)]
    np.testing.assert_array_equal(bits(got[0]), bits(np.array(want, F)))
    # the mask: shadowed -> black, alpha stays 1
    got, _ = Lg.shade_linear(rows[:1], hit[:1], p[:1], d[:1], sun, np.zeros((1, 1), np.uint8), None)
    np.testing.assert_array_equal(got, np.array([[0, 0, 0, 1]], F))
