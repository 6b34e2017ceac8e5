"""The path tracer's per-pixel state as include/mrt_hip.h states it (mrt_path_init, mrt_path_step, mrt_path_finish) restated in numpy
on bounce.py's sampler, lighting.py's Cook-Torrance terms and surface.py's rows: the radiance accumulation, the throughput weights of
sample_bounce, Russian roulette, the `active` flag, the five tone mappers and the gamma -- float32, one operation at a time, in the
order the header states, with pow01 in float64.  Test and tool plumbing (tests/test_path_*.py, tools/bench_path_frame.py): the
device's states, select and lobe bytes and finished frames must equal these byte for byte."""
import numpy as np

from . import bounce as B
from . import hemisphere as H
from . import lighting as Lg
from . import panorama as Pn
from . import types as T

F = np.float32
EPS7 = F(1e-7)
SURVIVAL_CAP = F(0.95)
GAMMA = F(1.0) / F(2.2)
# _hable_partial's constants: float products and one float quotient
HA, HB, HCB, HDE, HDF, HEF = F(0.15), F(0.50), F(0.10) * F(0.50), F(0.20) * F(0.02), F(0.20) * F(0.30), F(0.02) / F(0.30)


def first_draw(bounce):
    """draws of a pixel's stream before the lobe draw of bounce b: three per bounce, one more for every roulette before it"""
    return 3 * int(bounce) + max(0, int(bounce) - 2)


def init_state(n):
    st = np.zeros(n, T.PATH_STATE)
    st["throughput"], st["active"] = 1, 1
    return st


def hable_partial(x):
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        return ((x * (HA * x + HCB) + HDE) / (x * (HA * x + HB) + HDF)) - HEF


HABLE_WHITE = hable_partial(F(11.2))


def tonemap(c, mode):
    """tonemap_rgb's operator per channel, modes 0 .. 4"""
    c = np.asarray(c, dtype=F)
    with np.errstate(all="ignore"):
        if mode == 0:
            return c.copy()
        if mode == 1:
            return (c / (c + F(1))).astype(F)
        if mode == 2:
            return (hable_partial(c) / HABLE_WHITE).astype(F)
        if mode == 3:
            m = (c * (F(2.51) * c + F(0.03))) / (c * (F(2.43) * c + F(0.59)) + F(0.14))
            return np.where(m < F(0), F(0), np.where(m > F(1), F(1), m)).astype(F)
        if mode == 4:
            x = np.where(c < F(0), F(0), c).astype(F)
            x2 = x * x
            m = x2 / ((x2 + F(0.09) * x) + F(0.0009))
            return np.where(m > F(1), F(1), m).astype(F)
    raise ValueError("tonemap mode 0 .. 4")


def gamma(c):
    """pow(max(c, 0), 1 / 2.2f) through pow01"""
    c = np.asarray(c, dtype=F)
    return Lg.pow01(np.where(c < F(0), F(0), c).astype(F), GAMMA)


def path_finish(state, mode):
    """mrt_path_finish: [N, 4] float32"""
    out = np.ones((state.shape[0], 4), F)
    out[:, :3] = gamma(tonemap(state["radiance"], mode))
    return out


def surface_terms(rows):
    """f0 [N, 3] and the diffuse albedo [N, 3] of rows, as the lighting calls compute them"""
    one_m = F(1) - rows["metallic"]
    dielectric = (F(0.04) * rows["specular"]) * F(2)
    f0 = (dielectric * one_m)[:, None] + rows["albedo"] * rows["metallic"][:, None]
    diff = rows["albedo"] * one_m[:, None]
    return f0.astype(F), diff.astype(F)


def stream_seed(pixel_index, frame):
    return H._u32(H._u32(np.asarray(pixel_index, dtype=np.uint64) * np.uint64(1009)) + np.uint64((int(frame) * 6529 + 7) & H.M32))


def bounce_weights(rows, nrm, in_dirs, pixel_index, frame, bounce):
    """sample_bounce for N hit records: rows [N] T.SURFACE64, nrm [N, 3] the records' normals (faced here, as the cast faces them),
    in_dirs [N, 3] the incoming directions.  Returns a dict: w [N, 3] the throughput weight, valid [N] (ndl > 0), specular [N], sp,
    ndl, vh, h, u3 (the roulette draw, first_draw + 3)."""
    with np.errstate(all="ignore"):
        d = np.asarray(in_dirs, dtype=F)
        n = np.asarray(nrm, dtype=F).copy()
        flip = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] > F(0)
        n[flip] = -n[flip]
        seed = stream_seed(pixel_index, frame)
        k = first_draw(bounce)
        u0, u1, u2, u3 = (H.to_float(B.draw(seed, k + j)) for j in range(4))
        m, ro = B.clamp_surface(rows["metallic"], rows["roughness"])
        dirs, specular, sp, h = B.bounce_direction(n, d, m, ro, u0, u1, u2)
        ndl = (n[:, 0] * dirs[:, 0] + n[:, 1] * dirs[:, 1]) + n[:, 2] * dirs[:, 2]
        valid = ~(ndl <= F(0))
        v = B.normalized(-d)
        vh = np.maximum((v[:, 0] * h[:, 0] + v[:, 1] * h[:, 1]) + v[:, 2] * h[:, 2], F(0))
        ndh = Lg._fmax0((n[:, 0] * h[:, 0] + n[:, 1] * h[:, 1]) + n[:, 2] * h[:, 2])
        f0, diff = surface_terms(rows)
        ndv = rows["n_dot_v"]
        g = Lg.geometry_smith_ggx(ndv, ndl, ro)
        common = (g * vh) / (((ndv * ndh) * sp) + EPS7)
        w_spec = np.stack([Lg.fresnel_schlick(vh, f0[:, c]) * common for c in range(3)], axis=1)
        inv = F(1) / (F(1) - sp)
        w_diff = diff * inv[:, None]
        w = np.where(specular[:, None], w_spec, w_diff).astype(F)
    return dict(w=w, valid=valid, specular=specular, sp=sp, ndl=ndl.astype(F), vh=vh.astype(F), h=h, u3=u3, dirs=dirs)


def roulette(t):
    """surv = min(max(max(tr, tg), tb), 0.95f) with the reference's comparisons"""
    mx = np.where(t[:, 0] < t[:, 1], t[:, 1], t[:, 0])
    mx = np.where(mx < t[:, 2], t[:, 2], mx)
    return np.where(SURVIVAL_CAP < mx, SURVIVAL_CAP, mx).astype(F)


def path_step(state, rows, hit, nrm, in_dirs, direct, env, pixel_index, frame, bounce, max_bounces, info=None, panorama=None, emits=None):
    """mrt_path_step for N records: state [N] T.PATH_STATE (not modified), rows as mrt_resolve_surfaces wrote them, hit [N] bool, nrm
    [N, 3] the records' normals, in_dirs [N, 3] the incoming directions as given, direct [N, >= 3] what mrt_light_surfaces wrote with
    env == NULL, env one T.ENVIRONMENT row, pixel_index [N].  Returns (state', select [N] uint8, lobe [N] uint8, active count).  info: an
    optional dict that receives what happened to each entry, [N] bool each: missed, invalid (a sample below the surface), killed and
    survived (roulette), stopped (the last bounce).  panorama: (pixels [H, W, 4], energy) as resident (mrt_upload_panorama) or None -- the
    sky of a miss is then its sample.  emits: [N] bool or None -- mrt_path_step_emitters' rule, the emission line runs only where it is set
    (None: everywhere, mrt_path_step)."""
    N = state.shape[0]
    st = state.copy()
    hit = np.asarray(hit, dtype=bool)
    on = state["active"] != 0
    t, r = state["throughput"].astype(F).copy(), state["radiance"].astype(F).copy()
    alive = np.zeros(N, bool)
    lobe = np.full(N, B.LOBE_NONE, np.uint8)
    what = {k: np.zeros(N, bool) for k in ("missed", "invalid", "killed", "survived", "stopped")}
    with np.errstate(all="ignore"):
        miss = on & ~hit
        what["missed"] = miss
        what["stopped"] = on & hit & (bounce == max_bounces)
        if miss.any():
            miss_d = np.asarray(in_dirs, dtype=F)[miss]
            sky = Lg.sky_gradient(miss_d, env) if panorama is None else Pn.sky_panorama(panorama[0], panorama[1], miss_d)
            r[miss] = r[miss] + t[miss] * sky
        idx = np.nonzero(on & hit)[0]
        if idx.size:
            rw = rows[idx]
            tt, rr = t[idx], r[idx]
            f0, diff = surface_terms(rw)
            if emits is None:
                rr = rr + tt * rw["emission"]
            else:
                rr = np.where(np.asarray(emits, dtype=bool)[idx][:, None], rr + tt * rw["emission"], rr).astype(F)
            rr = rr + tt * np.asarray(direct, dtype=F)[idx, :3]
            if bounce == 0:
                amb = np.asarray(env["ambient"], dtype=F)
                rr = rr + ((tt * diff) * amb[None, :]) * F(env["ambient_energy"])
            r[idx] = rr
            if bounce != max_bounces:
                bw = bounce_weights(rw, np.asarray(nrm, dtype=F)[idx], np.asarray(in_dirs, dtype=F)[idx], np.asarray(pixel_index)[idx], frame, bounce)
                ok = bw["valid"].copy()
                what["invalid"][idx] = ~ok
                tt = np.where(ok[:, None], tt * bw["w"], tt).astype(F)
                if bounce >= 2:
                    surv = roulette(tt)
                    dead = ok & (bw["u3"] >= surv)
                    live = ok & ~dead
                    tt = np.where(live[:, None], tt * (F(1) / surv)[:, None], tt).astype(F)
                    what["killed"][idx], what["survived"][idx] = dead, live
                    ok = live
                t[idx] = tt
                alive[idx] = ok
                lobe[idx] = np.where(ok, np.where(bw["specular"], B.LOBE_SPECULAR, B.LOBE_DIFFUSE), B.LOBE_NONE)
    st["throughput"][on], st["radiance"][on] = t[on], r[on]
    st["active"][on] = alive[on]
    if info is not None:
        info.update(what)
    return st, alive.astype(np.uint8), lobe, int(alive.sum())


def trace_frame(bounces, env, pixel_index, frame, max_bounces):
    """CPUPathTracer's loop over records a caller supplies: `bounces` yields, for bounce 0, 1, ..., a dict with rows, hit, normal,
    direction (the incoming rays') and direct, each [N]; it is asked for bounce b + 1 only after bounce b's result is yielded back, so
    that a caller may trace the next rays from the select bytes.  Returns the list of (state, select, lobe, active count) per bounce
    run (the loop ends early when nothing is active, as the reference's does) -- the last state is what mrt_path_finish reads."""
    out = []
    state = None
    for b, rec in enumerate(bounces):
        if b > max_bounces:
            break
        if state is None:
            state = init_state(rec["rows"].shape[0])
        state, select, lobe, active = path_step(state, rec["rows"], rec["hit"], rec["normal"], rec["direction"], rec["direct"], env,
                                                pixel_index, frame, b, max_bounces)
        out.append((state, select, lobe, active))
        if active == 0:
            break
    return out
