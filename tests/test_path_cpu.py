"""The path tracer's per-pixel state without a device: the library exports the four entry points and the calls reject a null context;
the host-side refusals, the generator's jump, the tone mappers and the gamma (csrc/host/path_data_test.cpp); the gamma's sweep against
numpy's float64 power below and above 1; the numpy restatement (messyerraytracer_amd/path.py, what the GPU tests hold the kernels to
byte for byte) against values recorded from the reference's own sample_bounce, the loop body of CPUPathTracer::trace_frame
(cpu_path_tracer.h:113-194), its final pass (:203-221) and tonemap_rgb (tests/golden/path_reference.npz): bit for bit
wherever no libm value enters -- the accumulation, the sky of a miss, the diffuse weights, the roulette on them, the tone mappers --
and elsewhere within twice the largest difference measured, which is printed and asserted.

Measured on the fixture: over the specular tuples away from a decision the largest relative difference of a weight
channel is 1.144e-05 on 733 valid specular tuples, 609 of them bit for bit (the sincos difference §4.13 measured in the half vector,
through 1 - vh to the fifth power and, at grazing n . dir, through G's g1), asserted as 2.288e-05; the list of tuples within
that bound of a validity or roulette threshold holds exactly the 24 specular tuples placed at the roulette draw on purpose (1.2 % of the
2072, cap 2 %), one of which lands on the other side; the gamma differs from the rounded float64 power in 0 of the swept points below 1
and above it (worst 0 ulp) and from the host's powf in the recorded final pass by at most 1 ulp."""
import ctypes as C
import os
import subprocess

import numpy as np

from messyerraytracer_amd import bounce as B
from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import lighting as Lg
from messyerraytracer_amd import path as P
from messyerraytracer_amd import types as T

PTR = C.c_void_p(16)  # a pointer no call may dereference: every case below fails its checks first
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_reference.npz")
# §4.12's rule: a bound is twice the largest difference measured (the module's docstring has the measurements).
WEIGHT_BOUND = 2 * 1.144e-05
GAMMA_SWEEP_WORST_ULP = 0
GAMMA_RECORDED_WORST_ULP = 1


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def ulps(a, b):
    return np.abs(np.ascontiguousarray(a, dtype=F).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, dtype=F).view(np.int32).astype(np.int64))


def rel_diff(got, want):
    with np.errstate(all="ignore"):
        r = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.abs(want.astype(np.float64))
    return np.where(got == want, 0.0, r)


def test_exports_sizes_and_layouts():
    L = capi.load()
    for s in ("mrt_path_init", "mrt_path_step", "mrt_path_grid_step", "mrt_path_finish"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert (capi.STRUCT_PATH_STATE, capi.STRUCT_PATH_STEP_DESC) == (15, 16)
    assert L.mrt_struct_size(capi.STRUCT_PATH_STATE) == T.PATH_STATE.itemsize == 32
    assert L.mrt_struct_size(capi.STRUCT_PATH_STEP_DESC) == C.sizeof(capi.PathStepDesc) == 64
    assert L.mrt_struct_size(14) == 0 and L.mrt_struct_size(17) == 0
    assert [T.PATH_STATE.fields[n][1] for n in T.PATH_STATE.names] == [0, 12, 16, 28]
    assert [getattr(capi.PathStepDesc, n).offset for n, _ in capi.PathStepDesc._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56]
    st = P.init_state(3)
    assert st.view(np.uint32).reshape(3, 8).tolist() == [[0x3F800000] * 3 + [1, 0, 0, 0, 0]] * 3


def test_null_context_is_invalid():
    """(With a context, every bad argument is checked before any device work: test_path_gpu.py.)"""
    L = capi.load()
    desc = capi.PathStepDesc(0, 0, 4, 0, 16, 16, 16, 16, None, None)
    cam = capi.Camera()
    assert L.mrt_path_init(None, PTR, 1, 0) == capi.ERR_INVALID and L.mrt_path_init(None, None, 0, 0) == capi.ERR_INVALID
    assert L.mrt_path_step(None, PTR, PTR, PTR, 1, C.byref(desc), 0) == capi.ERR_INVALID
    assert L.mrt_path_step(None, None, None, None, 0, None, 1 << 20) == capi.ERR_INVALID
    assert L.mrt_path_grid_step(None, C.byref(cam), 4, 4, 0, 4, PTR, PTR, C.byref(desc), 0) == capi.ERR_INVALID
    assert L.mrt_path_finish(None, PTR, 1, 0, PTR, 0) == capi.ERR_INVALID and L.mrt_path_finish(None, PTR, 1, 9, None, 0) == capi.ERR_INVALID


def test_path_data_driver():
    exe = mbuild.build_path_data_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout


def test_first_draw_and_jump():
    assert [P.first_draw(b) for b in range(8)] == [0, 3, 6, 10, 14, 18, 22, 26] and P.first_draw(32) == 126
    seed = np.array([0, 1, 12345, 0xFFFFFFFF], np.uint64)
    stepped = B.H.draws(seed, 30)
    for k in (0, 3, 6, 9, 10, 13, 14, 26, 29):
        np.testing.assert_array_equal(B.draw(seed, k), stepped[:, k])


# ---- gamma ------------------------------------------------------------------------------------------------------------------------------

def test_gamma_sweep():
    """pow01 at e = 1 / 2.2f: every j * 2^-16 up to 1, 2^20 random bases in (1, 2^16], the ends"""
    rng = np.random.default_rng(2)
    above = (1 + rng.random(1 << 20) * (2.0 ** 16 - 1)).astype(F)
    above = above[above > 1]
    ends = np.array([0.0, 2.0 ** -149, 2.0 ** -126, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 11.2, 1e4, 2.0 ** 16, 3.4028234663852886e38], F)
    e = np.float64(P.GAMMA)
    for name, b in (("[0, 1]", (np.arange(65537, dtype=np.float64) / 65536).astype(F)), ("(1, 2^16]", above), ("ends", ends)):
        got = P.gamma(b)
        want = np.power(b.astype(np.float64), e).astype(F)
        d = ulps(got, want)
        print(f"gamma sweep {name}: {int((d > 0).sum())} of {d.size} points differ, worst {int(d.max())} ulp")
        assert int(d.max()) <= GAMMA_SWEEP_WORST_ULP
    assert P.gamma(F(-1)) == 0 and P.gamma(F(-0.0)) == 0 and P.gamma(F(1)) == 1 and P.gamma(F(np.inf)) == np.inf
    assert P.gamma(np.array([0.5], F)).dtype == F


# ---- the restatement against the reference's own functions -----------------------------------------------------------------------------

_FIXTURE = []


def fixture():
    """Every tuple through path_step once (grouped by bounce and last bounce: both are scalars of a step) and through bounce_weights."""
    if not _FIXTURE:
        g = np.load(GOLDEN)
        g = {k: g[k] for k in g.files}
        n = g["kind"].shape[0]
        rows = np.zeros(n, T.SURFACE64)
        for k in ("normal", "n_dot_v", "albedo", "metallic", "roughness", "specular"):
            rows[k] = g["in_" + k]
        rows["emission"] = g["in_emit"]
        env = np.zeros(1, T.ENVIRONMENT)
        env.view(F)[:13] = g["env"]
        state = np.zeros(n, T.PATH_STATE)
        state["throughput"], state["radiance"], state["active"], state["reserved"] = g["in_t"], g["in_acc"], g["in_active"], 0xABCD
        got = state.copy()
        select, lobe = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        w = np.zeros((n, 3), F)
        valid, spec = np.zeros(n, bool), np.zeros(n, bool)
        ndl, u3 = np.zeros(n, F), np.zeros(n, F)
        active_total = 0
        for b in np.unique(g["in_bounce"]):
            for last in (False, True):
                m = (g["in_bounce"] == b) & ((g["in_max_bounces"] == b) == last)
                if not m.any():
                    continue
                mb = int(g["in_max_bounces"][m][0])
                assert (g["in_max_bounces"][m] == mb).all()
                st, sel, lb, cnt = P.path_step(state[m], rows[m], g["in_hit"][m] != 0, g["in_normal"][m], g["in_dir"][m], g["in_direct"][m],
                                               env[0], g["pixel"][m], 0, int(b), mb)
                got[m], select[m], lobe[m] = st, sel, lb
                active_total += cnt
                bw = P.bounce_weights(rows[m], g["in_normal"][m], g["in_dir"][m], g["pixel"][m], 0, int(b))
                w[m], valid[m], spec[m], ndl[m], u3[m] = bw["w"], bw["valid"], bw["specular"], bw["ndl"], bw["u3"]
        g.update(rows=rows, env_row=env[0], state=state, got=got, select=select, lobe=lobe, w=w, valid=valid, spec=spec, ndl=ndl, u3=u3,
                 active_total=active_total)
        # what the reference alone says of each tuple: whether sample_bounce ran, its lobe (a diffuse weight is diff * inv exactly),
        # n . dir of the direction it made, the throughput after the weight and the survival probability made from it
        ran = (g["in_active"] != 0) & (g["in_hit"] != 0) & (g["in_bounce"] != g["in_max_bounces"])
        m_, ro_ = B.clamp_surface(rows["metallic"], rows["roughness"])
        sp = B.spec_prob(m_, ro_)
        ref_ndl = (g["in_normal"][:, 0] * g["out_br_dir"][:, 0] + g["in_normal"][:, 1] * g["out_br_dir"][:, 1]) + g["in_normal"][:, 2] * g["out_br_dir"][:, 2]
        tw = (g["in_t"] * g["out_w"]).astype(F)
        surv = P.roulette(tw)
        g.update(ran=ran, sp=sp, ref_ndl=ref_ndl.astype(F), ref_surv=surv)
        # the list: tuples whose validity or roulette decision lies within WEIGHT_BOUND of its threshold and rests on a libm value
        # (the direction of either lobe for validity; a specular weight for the roulette)
        near_valid = ran & (np.abs(ref_ndl) <= WEIGHT_BOUND)
        near_roulette = ran & (g["out_br_valid"] != 0) & spec & (g["in_bounce"] >= 2) & (np.abs(g["out_u3"].astype(np.float64) - surv) <= WEIGHT_BOUND * surv)
        g["near"] = near_valid | near_roulette
        _FIXTURE.append(g)
    return _FIXTURE[0]


def test_fixture_covers_what_it_must():
    g = fixture()
    kind, n = g["kind"], g["kind"].shape[0]
    assert 1900 <= n <= 2200
    for k, least in ((0, 1000), (1, 150), (2, 50), (3, 100), (4, 100), (5, 120), (6, 36), (7, 80), (8, 100), (9, 100), (10, 16)):
        assert (kind == k).sum() >= least, k
    ran, spec, b = g["ran"], g["spec"], g["in_bounce"]
    for bb in range(6):                                                       # every bounce index, both lobes at each
        assert (ran & spec & (b == bb)).sum() >= 20 and (ran & ~spec & (b == bb)).sum() >= 20, bb
    assert ((kind == 1) & (b == 0)).sum() >= 50 and ((kind == 1) & (b > 0)).sum() >= 50
    assert (g["in_hit"][kind == 1] == 0).all() and (g["out_active"][kind == 1] == 0).all()
    assert (g["in_active"][kind == 2] == 0).all()
    k3 = kind == 3
    assert (g["sp"][k3] == F(0.95)).sum() >= 50 and (g["sp"][k3] == F(0.05)).sum() >= 50
    assert (g["in_n_dot_v"][kind == 4] == F(0.001)).all()
    k5 = kind == 5
    u3, surv = g["out_u3"][k5], g["ref_surv"][k5]
    assert (~g["spec"][k5]).all() and (b[k5] >= 2).all() and (surv < F(0.95)).all()
    assert (u3 == surv).sum() >= 30 and (u3 == np.nextafter(surv, F(2))).sum() >= 30 and (u3 == np.nextafter(surv, F(0))).sum() >= 30
    assert (g["out_active"][k5] == (u3 < surv)).all()
    k6 = (kind == 6) & ~g["spec"] & (g["out_br_valid"] != 0)          # (a seed solved for its fourth draw may still draw the other lobe)
    u3 = g["out_u3"][k6]
    c = F(0.95)
    assert (g["ref_surv"][k6] == c).all() and (u3 == c).sum() >= 10 and (u3 == np.nextafter(c, F(0))).sum() >= 10 and (u3 == np.nextafter(c, F(2))).sum() >= 10
    assert sorted(np.unique(b[k6])) == [2, 3, 4, 5]
    assert ((g["ref_surv"] == c) & ran & (b >= 2)).sum() >= 100 and ((g["ref_surv"] < c) & ran & (b >= 2)).sum() >= 300
    assert (g["in_bounce"][kind == 7] == g["in_max_bounces"][kind == 7]).all() and sorted(np.unique(b[kind == 7])) == list(range(6))
    assert (g["out_active"][kind == 7] == 0).all()
    assert (g["in_emit"][kind == 8] > 0).all()
    roul = ran & (g["out_br_valid"] != 0) & (b >= 2)
    assert (roul & (g["out_active"] == 0)).sum() >= 100 and (roul & (g["out_active"] != 0)).sum() >= 100   # kills and survivals
    assert (ran & (g["out_br_valid"] == 0)).sum() >= 5                                                      # invalid samples
    assert np.isfinite(g["out_t"]).all() and np.isfinite(g["out_acc"]).all()
    on = g["in_active"] != 0                                                   # (an inactive pixel's ray is left as it was)
    assert (g["out_local_active"] == g["out_active"]).all() and (g["out_next_valid"][on] == g["out_active"][on]).all()
    # the final pass: five modes on 0, denormals, around 1, 11.2 and 1e4, negative inputs
    fr, fm = g["final_radiance"], g["final_mode"]
    for mode in range(5):
        v = fr[fm == mode]
        for x in (0.0, 1e-45, 1e-40, 1.0, 11.2, 1e4, -0.5, -1e4):
            assert (v == F(x)).any(), (mode, x)
        assert (v == np.nextafter(F(1), F(0))).any() and (v == np.nextafter(F(11.2), F(20))).any()


def test_accumulation_and_sky_equal_the_reference_bit_for_bit():
    """Every tuple's radiance: emission, direct, the ambient term of bounce 0, the sky of a miss -- no libm value enters."""
    g = fixture()
    np.testing.assert_array_equal(bits(g["got"]["radiance"]), bits(g["out_acc"]))
    miss = (g["in_hit"] == 0)
    sky = Lg.sky_gradient(g["in_dir"][miss], g["env_row"])
    np.testing.assert_array_equal(bits(sky), bits(g["out_sky"][miss]))
    untouched = g["in_active"] == 0
    np.testing.assert_array_equal(g["got"][untouched].view(np.uint32), g["state"][untouched].view(np.uint32))
    assert (g["select"][untouched] == 0).all() and (g["lobe"][untouched] == 0).all()
    assert (g["got"]["reserved"] == 0xABCD).all()                              # carried through


def test_lobe_and_draws_equal_the_reference():
    g = fixture()
    ran = g["ran"]
    np.testing.assert_array_equal(bits(g["u3"][ran]), bits(g["out_u3"][ran]))
    # a diffuse weight is diff * inv exactly and a specular one carries F: the recorded weight tells the lobe where it is valid
    ok = ran & (g["out_br_valid"] != 0) & ~g["near"]
    diffuse_w = (g["rows"]["albedo"] * (F(1) - g["rows"]["metallic"])[:, None]) * (F(1) / (F(1) - g["sp"]))[:, None]
    is_diffuse = (bits(diffuse_w) == bits(g["out_w"])).all(axis=1)
    assert (is_diffuse[ok] == ~g["spec"][ok]).all()


def test_diffuse_tuples_equal_the_reference_bit_for_bit():
    """Weights, throughput, roulette and the active flag of every tuple that took the diffuse lobe (or never sampled)."""
    g = fixture()
    k = ~g["near"] & ~(g["ran"] & g["spec"])
    assert k.sum() >= 1000 and (k & g["ran"]).sum() >= 500
    np.testing.assert_array_equal(bits(g["got"]["throughput"][k]), bits(g["out_t"][k]))
    np.testing.assert_array_equal(g["got"]["active"][k], g["out_active"][k])
    np.testing.assert_array_equal(g["select"][k], g["out_active"][k].astype(np.uint8))
    kv = k & g["ran"] & (g["out_br_valid"] != 0)
    np.testing.assert_array_equal(bits(g["w"][kv]), bits(g["out_w"][kv]))
    assert (g["valid"][k & g["ran"]] == (g["out_br_valid"][k & g["ran"]] != 0)).all()
    assert (g["lobe"][k & (g["out_active"] != 0)] == B.LOBE_DIFFUSE).all()


def test_specular_tuples_within_the_sincos_bound():
    g = fixture()
    k = ~g["near"] & g["ran"] & g["spec"]
    assert k.sum() >= 500
    assert (g["valid"][k] == (g["out_br_valid"][k] != 0)).all()
    kv = k & g["valid"]
    r = rel_diff(g["w"][kv], g["out_w"][kv])
    assert np.isfinite(r).all()
    print(f"specular tuples: {kv.sum()} valid, {(r == 0).all(axis=1).sum()} bit for bit, largest relative difference of a weight channel {r.max():.3e}")
    assert r.max() <= WEIGHT_BOUND
    np.testing.assert_array_equal(g["got"]["active"][k], g["out_active"][k])
    rt = rel_diff(g["got"]["throughput"][k], g["out_t"][k])
    print(f"specular tuples: largest relative difference of the throughput after the step {rt.max():.3e}")
    assert rt.max() <= 2 * WEIGHT_BOUND                                         # a weight, then 1 / surv made from it
    assert (g["lobe"][k & (g["out_active"] != 0)] == B.LOBE_SPECULAR).all()


def test_tuples_at_a_decision():
    """Validity or roulette within the bound of its threshold, resting on a libm value: the list is at most 2 % of the fixture by the
    reference's figures alone, and on it each side holds one of the two outcomes: the recorded state, or the state of the other
    decision (ended with the throughput as it stood then)."""
    g = fixture()
    near = g["near"]
    n = near.shape[0]
    other = sum(int(g["got"]["active"][i] != g["out_active"][i]) for i in np.nonzero(near)[0])
    print(f"at a decision: {near.sum()} tuples of {n}, {other} on the other side")
    assert 16 <= near.sum() <= n // 50
    assert (g["kind"][near] == 10).all()                                       # only the ones put there on purpose
    for i in np.nonzero(near)[0]:
        got_t, got_a = g["got"]["throughput"][i], g["got"]["active"][i]
        if got_a == g["out_active"][i]:
            assert rel_diff(got_t, g["out_t"][i]).max() <= 2 * WEIGHT_BOUND
        else:
            tw = (g["in_t"][i] * g["out_w"][i]).astype(F)
            alt = [g["in_t"][i], tw, (tw * (F(1) / g["ref_surv"][i])).astype(F)]
            assert min(rel_diff(got_t, a).max() for a in alt) <= 2 * WEIGHT_BOUND
        np.testing.assert_array_equal(bits(g["got"]["radiance"][i]), bits(g["out_acc"][i]))


def test_active_count_is_the_sum_of_select():
    g = fixture()
    assert g["active_total"] == int(g["select"].sum()) and g["active_total"] > 500


# ---- the final pass ---------------------------------------------------------------------------------------------------------------------

def test_tone_mappers_equal_the_reference_bit_for_bit():
    """tonemap_rgb has no libm call: with the gamma taken out (mode by mode, the recorded frame against the restatement's tone-mapped
    value pushed through the host's own powf), every channel agrees to the bit; hand-written values pin the operand order."""
    g = fixture()
    libm = C.CDLL(None)
    libm.powf.restype, libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    for mode in range(5):
        m = g["final_mode"] == mode
        tm = P.tonemap(g["final_radiance"][m], mode)
        with np.errstate(all="ignore"):
            base = np.where(tm < 0, F(0), tm).astype(F)
        want = np.array([libm.powf(float(x), float(P.GAMMA)) for x in base.ravel()], F).reshape(base.shape)
        np.testing.assert_array_equal(bits(want), bits(g["final_rgba"][m, :3]))
    assert (g["final_rgba"][:, 3] == 1).all()
    assert P.tonemap(F(1), 1) == F(0.5) and P.tonemap(F(11.2), 2) == F(1) and P.tonemap(F(1e4), 3) == F(1) and P.tonemap(F(-2), 4) == F(0)
    assert bits(P.tonemap(F(1), 3)) == bits((F(2.51) + F(0.03)) / ((F(2.43) + F(0.59)) + F(0.14)))
    assert bits(P.tonemap(F(1), 4)) == bits(F(1) / ((F(1) + F(0.09)) + F(0.0009)))


def test_finished_frame_within_the_gamma_bound():
    g = fixture()
    worst = 0
    for mode in range(5):
        m = g["final_mode"] == mode
        st = np.zeros(int(m.sum()), T.PATH_STATE)
        st["radiance"] = g["final_radiance"][m]
        got = P.path_finish(st, mode)
        assert (got[:, 3] == 1).all() and got.dtype == F
        d = ulps(got[:, :3], g["final_rgba"][m, :3])
        worst = max(worst, int(d.max()))
    print(f"finished frame against the reference's pow: worst {worst} ulp")
    assert worst <= GAMMA_RECORDED_WORST_ULP


def test_trace_frame_runs_the_loop():
    """The loop's plumbing on hand-made records: it stops when nothing is active, and never runs past max_bounces."""
    n = 4
    rows = np.zeros(n, T.SURFACE64)
    rows["normal"], rows["n_dot_v"], rows["albedo"], rows["roughness"], rows["specular"] = (0, 1, 0), 1, 0.5, 0.5, 0.5
    rec = dict(rows=rows, hit=np.array([True, True, False, True]), normal=rows["normal"], direction=np.tile(F([0, -1, 0]), (n, 1)),
               direct=np.full((n, 4), 0.25, F))
    env = np.zeros(1, T.ENVIRONMENT)[0]
    env["sky_zenith"], env["sky_horizon"], env["sky_ground"], env["ambient"], env["ambient_energy"] = (0.25, 0.5, 1), (0.5, 0.5, 0.5), (0.125, 0, 0.25), (1, 0.5, 2), 0.5
    asked = []

    def bounces():
        for b in range(10):
            asked.append(b)
            yield rec

    out = P.trace_frame(bounces(), env, np.arange(n), 3, 2)
    assert len(out) == 3 and asked == [0, 1, 2] and out[-1][3] == 0 and (out[-1][0]["active"] == 0).all()
    st0 = out[0][0]
    # the miss: the sky straight down (t = 0: the ground colour) times throughput 1; the hits: direct 0.25 + ambient ((1 * 0.5) * amb) * 0.5
    np.testing.assert_array_equal(st0["radiance"][2], F([0.125, 0, 0.25]))
    np.testing.assert_array_equal(st0["radiance"][0], F([0.25 + 0.25, 0.25 + 0.125, 0.25 + 0.5]))
    assert st0["active"][2] == 0 and out[0][1][2] == 0 and out[0][3] == int(out[0][1].sum())
    none = P.trace_frame(iter([dict(rec, hit=np.zeros(n, bool))]), env, np.arange(n), 0, 4)
    assert len(none) == 1 and none[0][3] == 0
