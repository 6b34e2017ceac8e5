"""Every walk on trees as deep as its traversal stack allows ("Stack capacities"): the chain scene of tests/deep_tree.py,
a caller's tree of depth n with n triangles, uploaded at the depths where stack_depth == depth (8, 16, 64) and one below and above a
multiple of 8 (9, 17, 63; with stack_override == depth for the same exactness, and without), cast on every kernel form -- named by
mrt_last_kernel_variant -- closest hit, any hit with BOOL_OUT and TOKEN_OUT expanded again, and held to the brute-force test of every
triangle (the oracle's walk over the same nodes equals it on every ray: test_deep_trees_cpu.py).  Forward ray j's answer comes out of
stack entry j, so a lost or overwritten entry is a wrong record.  Every context has MRT_POISON_OUTPUT set.  Counting builds must report
exactly the high-water mark the push rule restated in Python gives (deep_tree.high_water), not merely stay below stack_need."""
import numpy as np
import pytest

import deep_tree as dt
import layout_check as lc
from messyerraytracer_amd import capi, synth, types as T
from messyerraytracer_amd.shadow import shadow_rays
from oracle import pyoracle as po
import parity

pytestmark = pytest.mark.gpu

N_RAYS = 4096          # per ray set (the grid: 64 x 64)
W = H = dt.GRID_W
# the ray sets of a form: mrt_cast of the axis rays plain and declared COHERENT; the interleaved rays the same two ways (a packet kernel
# only gets a batch declared coherent, and then each packet of 64 holds both directions); mrt_cast_grid; the bounded axis rays
SETS = ("axis", "coherent", "interleaved", "interleaved_coherent", "grid", "bounded")

PLAIN_FORMS = {
    "LANE": dict(kernel=capi.KERNEL_LANE), "PACKET": dict(kernel=capi.KERNEL_PACKET), "PACKET_ASM": dict(kernel=capi.KERNEL_PACKET_ASM),
    "PACKET_ROWS": dict(kernel=capi.KERNEL_PACKET_ROWS), "AUTO": dict(kernel=capi.KERNEL_AUTO),
    "DUAL_64_1": dict(kernel=capi.KERNEL_PACKET_DUAL, packet_wg=64, packet_cull=1),
    "DUAL_64_2": dict(kernel=capi.KERNEL_PACKET_DUAL, packet_wg=64, packet_cull=2),
    "DUAL_256_1": dict(kernel=capi.KERNEL_PACKET_DUAL, packet_wg=256, packet_cull=1),
    "DUAL_256_2": dict(kernel=capi.KERNEL_PACKET_DUAL, packet_wg=256, packet_cull=2),
}
if capi.kernel_available(capi.KERNEL_PACKET_QUAD):   # builds with MRT_WITH_QUAD=1 only
    PLAIN_FORMS["PACKET_QUAD"] = dict(kernel=capi.KERNEL_PACKET_QUAD)
# the persistent walks: stack_override is their LDS depth; below the scene's need the rest spills to HBM rows
PERSISTENT_FORMS = {f"{name}_{lds}": dict(kernel=k, stack_override=lds)
                    for name, k in (("LANE_PERSISTENT", capi.KERNEL_LANE_PERSISTENT), ("LANE4_PERSISTENT", capi.KERNEL_LANE4_PERSISTENT),
                                    ("LANE8_PERSISTENT", capi.KERNEL_LANE8_PERSISTENT)) for lds in (4, 16, 64)}
EXACT_DEPTHS = (8, 16, 64)      # stack_depth == depth: rounding leaves no slack
ODD_DEPTHS = (9, 17, 63)
CASES = ([(f, n, False) for f in PLAIN_FORMS for n in EXACT_DEPTHS + ODD_DEPTHS] + [(f, n, True) for f in PLAIN_FORMS for n in ODD_DEPTHS] +
         [(f, n, False) for f in PERSISTENT_FORMS for n in EXACT_DEPTHS + ODD_DEPTHS])

# form -> the instantiation after each of SETS ({A}: "true" in any-hit mode, "false" otherwise; a TOKEN_OUT cast runs the closest-hit
# one).  Printed by this file's own casts; a form that falls back to another kernel on so small a batch is listed as what it runs.
_LANE, _PACKET, _ASM = "trace_lane_kernel<{A}, false>", "trace_packet_kernel<{A}, false>", "trace_packet_asm_kernel<{A}, false, true>"


def _rows(packets, wg, cull):
    k = f"trace_packet_rows_kernel<{{A}}, false, {packets}, {wg}, {cull}>"
    return (_LANE, k, _LANE, k, k, _LANE)      # a batch not declared coherent goes to the lane kernel


def _persistent(width):
    k = f"trace_lane_persistent_kernel<{{A}}, {width}, false, false>"
    return (k, k, k, k, _LANE, k)              # a grid cast has no persistent form


EXPECT = {
    "LANE": (_LANE,) * 6, "PACKET": (_PACKET,) * 6, "PACKET_ASM": (_ASM,) * 6, "PACKET_ROWS": _rows(1, 256, "false"),
    "AUTO": (_LANE, _LANE, _LANE, _LANE, _ASM, _LANE),   # 4 096 rays: too few for packets, but a grid this small goes in sixteenths of tiles
    "DUAL_64_1": _rows(2, 64, "false"), "DUAL_64_2": _rows(2, 64, "true"), "DUAL_256_1": _rows(2, 256, "false"), "DUAL_256_2": _rows(2, 256, "true"),
    "LANE_PERSISTENT": _persistent(2), "LANE4_PERSISTENT": _persistent(4), "LANE8_PERSISTENT": _persistent(8),
}


def names_of(form):
    if form in EXPECT:
        return EXPECT[form]
    name, lds = form.rsplit("_", 1)
    return EXPECT[name]   # the persistent forms: the same instantiation at every LDS depth


WANT = {}


def inputs(n):
    """chain(n), its ray sets and brute force's answers: made once, never changed"""
    if n in WANT:
        return WANT[n]
    s = dt.prepared(n)
    o, f, fov = dt.grid_camera(n)
    sets = {"axis": dt.axis_rays(n, N_RAYS), "interleaved": dt.interleaved_rays(n, N_RAYS), "bounded": dt.bounded_rays(n, N_RAYS),
            "grid": po.grid_rays(o, f, W, H, fov)}
    sets["coherent"], sets["interleaved_coherent"] = sets["axis"], sets["interleaved"]
    want = {k: po.trace_brute(s["tris"], r) for k, r in sets.items()}
    masked = po.trace_brute(s["tris"], sets["axis"], query_mask=dt.LAYERS[1])
    assert (want["axis"]["prim_id"][:n] == dt.chain_ids(n)).all() and (masked["prim_id"] != want["axis"]["prim_id"]).any()
    WANT[n] = dict(s=s, sets=sets, want=want, masked=masked, cam=(o, f, fov))
    return WANT[n]


class Dev:
    """device buffers of one context, freed at the end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.device_alloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def put(self, arr):
        p = self.alloc(arr.nbytes)
        self.ctx.h2d(p, arr)
        return p

    def get(self, p, n, dtype):
        out = np.zeros(n, dtype=dtype)
        self.ctx.d2h(out, p)
        return out

    def free(self):
        for p in self.ptrs:
            self.ctx.device_free(p)
        self.ptrs = []


def upload_chain(c, n):
    s = dt.prepared(n)
    c.upload_scene(s["tris"], s["nodes"], s["prim_idx"])
    info = c.scene_info()
    assert info["stack_need"] == n and info["n_tris"] == n, info
    return s


def cast_set(c, dev, inp, name, what):
    """One ray set in the three modes, each held to brute force.  Returns {mode: instantiation name}."""
    rays, want = inp["sets"][name], inp["want"][name]
    n_rays, hit = rays.shape[0], want["prim_id"] >= 0
    seen = {}
    if name == "grid":
        cam = capi.camera_look(*inp["cam"][:2], W, H, inp["cam"][2])
        got = c.cast_grid(cam, W, H)
        seen["nearest"] = c.last_kernel_variant()
        parity.assert_exact(got, want, f"{what} grid: {seen['nearest']}")
        lit = c.cast_grid(cam, W, H, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        seen["any"] = c.last_kernel_variant()
        assert np.array_equal(lit.astype(bool), hit), f"{what} grid any-hit: {seen['any']}"
        tok = c.cast_grid(cam, W, H, flags=capi.FLAG_TOKEN_OUT)
        seen["token"] = c.last_kernel_variant()
        d_tok, d_hits = dev.put(tok), dev.alloc(n_rays * 32)
        c.expand_grid_tokens(cam, W, H, 0, H, d_tok, d_hits)
    else:
        flags = capi.FLAG_COHERENT if name.endswith("coherent") else 0
        got = c.cast(rays, flags=flags)
        seen["nearest"] = c.last_kernel_variant()
        parity.assert_exact(got, want, f"{what} {name}: {seen['nearest']}")
        lit = c.cast(rays, mode=capi.MODE_ANY_HIT, flags=flags | capi.FLAG_BOOL_OUT)
        seen["any"] = c.last_kernel_variant()
        assert np.array_equal(lit.astype(bool), hit), f"{what} {name} any-hit: {seen['any']}"
        tok = c.cast(rays, flags=flags | capi.FLAG_TOKEN_OUT)
        seen["token"] = c.last_kernel_variant()
        d_rays, d_tok, d_hits = dev.put(rays), dev.put(tok), dev.alloc(n_rays * 32)
        c.expand_tokens(d_rays, d_tok, d_hits, n_rays)
    assert np.array_equal(tok != capi.TOKEN_MISS, hit), f"{what} {name} tokens: {seen['token']}"
    c.synchronize()
    parity.assert_exact(dev.get(d_hits, n_rays, T.HIT32), want, f"{what} {name} tokens expanded: {seen['token']}")
    dev.free()
    return seen


def check_names(seen, form, what):
    if form == "PACKET_QUAD":   # (only in builds with MRT_WITH_QUAD=1: held to brute force like every form, its instantiations not listed)
        return
    for name, expect in zip(SETS, names_of(form)):
        for mode, a in (("nearest", "false"), ("any", "true"), ("token", "false")):
            assert seen[name][mode] == expect.replace("{A}", a), (what, name, mode, seen[name][mode])


@pytest.fixture
def poison(monkeypatch):
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")   # every output starts as a pattern no kernel writes: a record nobody wrote shows


@pytest.mark.parametrize("form,n,override", CASES, ids=[f"{f}-n{n}{'-override' if o else ''}" for f, n, o in CASES])
def test_every_form_walks_the_chain_to_its_bottom(built, poison, form, n, override):
    opts = dict(PLAIN_FORMS.get(form) or PERSISTENT_FORMS[form])
    if override:
        opts["stack_override"] = n     # api.hip base_params: exactly n entries per lane instead of n rounded up to 8
    inp = inputs(n)
    what = f"chain({n}) {form}{' override' if override else ''}"
    c = capi.Context(0, **opts)
    dev = Dev(c)
    try:
        upload_chain(c, n)
        seen = {name: cast_set(c, dev, inp, name, what) for name in SETS}
        # the even triangles masked out: the expected triangle moves one entry down the stack
        parity.assert_exact(c.cast(inp["sets"]["axis"], query_mask=dt.LAYERS[1]), inp["masked"], f"{what} masked")
        parity.assert_exact(c.cast(inp["sets"]["axis"], query_mask=dt.LAYERS[1], flags=capi.FLAG_COHERENT), inp["masked"], f"{what} masked coherent")
        print(f"NAMES {form} {n} {int(override)} " + " | ".join(seen[name][m] for name in SETS for m in ("nearest", "any")))
        check_names(seen, form, what)
    finally:
        dev.free()
        c.close()


# ---- counting builds: the high-water mark itself -----------------------------------------------------------------------------------
def records_high_water(variant):
    """the instantiations that write kCntMaxStack: the plain lane kernel (lane_walk.h) and the row walks (packet_rows_kernel.h);
    the C++ packet kernel, the 64-ray asm walk and the persistent kernels keep no such mark"""
    return variant.startswith("trace_lane_kernel<") or variant.startswith("trace_packet_rows_kernel<")


COUNT_FORMS = ["LANE", "PACKET", "PACKET_ASM", "PACKET_ROWS", "DUAL_64_1", "DUAL_64_2", "DUAL_256_1", "DUAL_256_2", "AUTO",
               "LANE_PERSISTENT_4", "LANE4_PERSISTENT_16", "LANE8_PERSISTENT_64"]


@pytest.mark.parametrize("n", EXACT_DEPTHS + ODD_DEPTHS, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("form", COUNT_FORMS)
def test_counting_builds_report_the_restated_high_water_mark(built, poison, form, n):
    """max_stack_depth is a running maximum of the context: shallow batch first (backward rays: 2 entries), then the deep ones (n).
    Exactly the restated figure, whichever instantiation ran: the row walks used to report 7 of 8, 15 of 16 or 1 of 2 on some launches
    (their mark was read one wait state too early after the push: MRT_ROWS_CNT_P, packet_rows_kernel.h), which `<= stack_need` let pass."""
    opts = dict(PLAIN_FORMS.get(form) or PERSISTENT_FORMS[form])
    inp = inputs(n)
    s = inp["s"]
    back, fwd = dt.backward_rays(n, N_RAYS), dt.forward_rays(n, N_RAYS)
    want_back, want_fwd = po.trace_brute(s["tris"], back), po.trace_brute(s["tris"], fwd)
    restated = {"backward": dt.batch_high_water(s, 2, back), "forward": dt.batch_high_water(s, 2, fwd),
                "grid": dt.batch_high_water(s, 2, inp["sets"]["grid"][::61])}
    assert restated == {"backward": 2, "forward": n, "grid": n}
    c = capi.Context(0, count_visits=True, **opts)
    try:
        upload_chain(c, n)
        cam = capi.camera_look(*inp["cam"][:2], W, H, inp["cam"][2])
        expect, marks = 0, []
        for batch, rays, want, flags in (("backward", back, want_back, capi.FLAG_COHERENT), ("backward", back, want_back, 0),
                                         ("forward", fwd, want_fwd, capi.FLAG_COHERENT), ("forward", fwd, want_fwd, 0),
                                         ("grid", None, inp["want"]["grid"], 0)):
            got = c.cast_grid(cam, W, H) if rays is None else c.cast(rays, flags=flags)
            variant = c.last_kernel_variant()
            parity.assert_exact(got, want, f"counting chain({n}) {form} {batch} flags={flags}: {variant}")
            if records_high_water(variant):
                expect = max(expect, restated[batch])
            have = c.stats()["max_stack_depth"]
            marks.append((batch, flags, variant, have))
            print(f"HIGHWATER {form} {n} {batch} flags={flags} {variant}: {have} (restated so far {expect})")
            assert have == expect, (form, n, marks)
        assert c.stats()["hits"] > 0
    finally:
        c.close()


# ---- the bound itself ------------------------------------------------------------------------------------------------------------------
def test_chain_65_is_refused_and_chain_64_is_walked(built, poison):
    s65, inp = dt.prepared(65), inputs(64)
    for kernel in (capi.KERNEL_AUTO, capi.KERNEL_LANE, capi.KERNEL_LANE8_PERSISTENT):
        c = capi.Context(0, kernel=kernel)
        try:
            with pytest.raises(capi.MrtError) as e:
                c.upload_scene(s65["tris"], s65["nodes"], s65["prim_idx"])
            assert e.value.status == capi.ERR_UNSUPPORTED
            assert not c.is_available()          # no half-installed scene
            with pytest.raises(capi.MrtError) as e:
                c.cast(inp["sets"]["axis"])
            assert e.value.status == capi.ERR_NO_SCENE
            upload_chain(c, 64)                  # ... and the context still works
            parity.assert_exact(c.cast(inp["sets"]["axis"]), inp["want"]["axis"], f"chain(64) after a refused chain(65), kernel {kernel}")
        finally:
            c.close()


# ---- neighbours: a stack that overruns writes into the next wave's region ------------------------------------------------------------
@pytest.mark.parametrize("n", EXACT_DEPTHS + (63,), ids=lambda n: f"n{n}")
@pytest.mark.parametrize("form", ["LANE", "PACKET", "PACKET_ASM", "PACKET_ROWS", "DUAL_64_2", "DUAL_256_1", "LANE_PERSISTENT_64", "LANE8_PERSISTENT_4"])
def test_full_workgroups_at_the_bottom_leave_their_neighbours_alone(built, poison, form, n):
    """8 192 rays that all hold n entries at once: every workgroup has four waves at the bottom of the chain together (declared
    coherent: 64 rays per wave; undeclared: the lane kernel gives so small a batch a wave per ray, four to a workgroup all the same).
    Then backward rays alone in the same context: a sentinel overwritten in a neighbouring wave's region shows in either."""
    opts = dict(PLAIN_FORMS.get(form) or PERSISTENT_FORMS[form])
    s = dt.prepared(n)
    fwd, back = dt.forward_rays(n, 8192), dt.backward_rays(n, 8192)
    want_fwd, want_back = po.trace_brute(s["tris"], fwd), po.trace_brute(s["tris"], back)
    c = capi.Context(0, **opts)
    try:
        upload_chain(c, n)
        for flags in (capi.FLAG_COHERENT, 0):
            parity.assert_exact(c.cast(fwd, flags=flags), want_fwd, f"chain({n}) {form} 8192 forward flags={flags}: {c.last_kernel_variant()}")
            parity.assert_exact(c.cast(back, flags=flags), want_back, f"chain({n}) {form} 8192 backward flags={flags}: {c.last_kernel_variant()}")
            lit = c.cast(fwd, mode=capi.MODE_ANY_HIT, flags=flags | capi.FLAG_BOOL_OUT)
            assert lit.all()
    finally:
        c.close()


# ---- refit: the bottom-up box pass over a 63-long serial chain ------------------------------------------------------------------------
SCALE, SHIFT = np.float32([2.0, 0.5, 0.5]), np.float32([3.0, 0.25, -0.125])


def moved(rays):
    """the rays of the chain for the chain moved by p -> p * SCALE + SHIFT (directions are +-x: kept; distances double)"""
    out = rays.copy()
    out["origin"] = rays["origin"] * SCALE + SHIFT
    finite = rays["t_max"] < T.FLT_MAX
    out["t_max"][finite] = rays["t_max"][finite] * SCALE[0]
    out["t_min"] = np.where(rays["t_min"] > 0.01, rays["t_min"] * SCALE[0], rays["t_min"])
    return out


@pytest.mark.parametrize("form", ["LANE", "DUAL_64_2", "LANE8_PERSISTENT_4"])
def test_refit_of_the_chain_keeps_its_depth_and_its_answers(built, poison, form):
    n = 64
    opts = dict(PLAIN_FORMS.get(form) or PERSISTENT_FORMS[form])
    inp = inputs(n)
    verts1 = (dt.chain_verts(n) * SCALE + SHIFT).astype(np.float32)
    tris1 = dt.chain_triangles(capi.make_triangles, n, verts1)
    o, f, fov = inp["cam"]
    o1 = tuple(float(x) for x in np.float32(o) * SCALE + SHIFT)
    sets = {"axis": moved(inp["sets"]["axis"]), "bounded": moved(inp["sets"]["bounded"]), "interleaved": moved(inp["sets"]["interleaved"])}
    c = capi.Context(0, **opts)
    try:
        upload_chain(c, n)
        c.refit_scene(tris1)
        snap = c.debug_snapshot()
        findings = lc.check_flat(snap, tris1, leaf_boxes="device")
        assert not findings, lc.summary(findings)
        assert snap["depth"] == n and c.scene_info()["stack_need"] == n
        for name, rays in sets.items():
            want = po.trace_brute(tris1, rays)
            assert (want["prim_id"] >= 0).any()
            for flags in (0, capi.FLAG_COHERENT):
                parity.assert_exact(c.cast(rays, flags=flags), want, f"refit chain {form} {name} flags={flags}: {c.last_kernel_variant()}")
        cam = capi.camera_look(o1, f, W, H, fov)
        want = po.trace_brute(tris1, po.grid_rays(o1, f, W, H, fov))
        assert len(set(want["prim_id"])) > 8
        parity.assert_exact(c.cast_grid(cam, W, H), want, f"refit chain {form} grid: {c.last_kernel_variant()}")
    finally:
        c.close()


# ---- a deep tree built on the device -----------------------------------------------------------------------------------------------------
# The Morton chain of test_device_build_gpu.py (one triangle per key bit: a 63-deep chain in the radix tree, the point that fixes the
# scene's extent, then coincident triangles at the origin, which the radix tree splits by index below the chain's end).  Read on the
# device, once: with no coincident triangle (64 triangles) stack_need is 63, with one (65 triangles) it is 64 and the tree is accepted,
# with two (66 triangles) and with every longer scene tried, up to the 128 triangles of the test named above, the build is refused.
M_ACCEPTED, NEED_ACCEPTED = 1, 64


def morton_chain(m):
    pts = []
    for k in range(63):
        bit = 62 - k                      # key bit 3t + axis holds bit t of that axis' grid coordinate
        p = [0.0, 0.0, 0.0]
        p[bit % 3] = float(1 << (bit // 3))
        pts.append(p)
    pts.append([float((1 << 21) - 1)] * 3)   # fixes the scene extent at 2^21 - 1 grid cells of size 1
    pts += [[0.0, 0.0, 0.0]] * m
    c0 = np.array(pts, dtype=np.float32)
    v = np.zeros((c0.shape[0], 3, 3), dtype=np.float32)
    v[:, 0] = c0 + np.float32([0.1, 0.1, 0.1]); v[:, 1] = c0 + np.float32([0.4, 0.1, 0.2]); v[:, 2] = c0 + np.float32([0.1, 0.4, 0.3])
    return v


def morton_rays(v, seed=7):
    row = np.zeros(256, dtype=T.RAY32)
    # (that test's row, moved by 0.005 in x and y: there every hundredth ray ran exactly along a triangle's edge, where a walk and brute force may differ)
    row["origin"] = np.float32([0.205, 0.205, -5.0]) + np.float32([1.0, 0.0, 0.0]) * (np.arange(256, dtype=np.float32)[:, None] * 0.01)
    row["direction"] = [0.0, 0.0, 1.0]
    row["t_min"], row["t_max"] = 0.001, T.FLT_MAX
    inc = synth.incoherent_rays(4096, seed)
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    reach = np.abs(inc["origin"]).max()
    inc["origin"] = (inc["origin"] / reach * (hi - lo) * 0.5 + (hi + lo) * 0.5).astype(np.float32)   # scaled to the scene's box
    # ... which hit next to nothing of 65 small triangles spread over 2^21 units: 32 rays aimed at a point inside each triangle, from
    # all directions and from 1 to 50 units away.  Only triangles within 2^16 of the origin are aimed at: further out the spacing of
    # floats nears the size of a triangle, the slab test of its few-ulp box is ill-conditioned, and a walk may cull what brute force
    # hits (the oracle's walk does, on its own tree, from 2^20 on): such a ray is a wrong input, not a finding.
    rng = np.random.default_rng(seed)
    v = v[np.abs(v).max(axis=(1, 2)) < 65536.0]
    n, per = v.shape[0], 32
    a, b = rng.uniform(0.1, 0.4, (2, n, per, 1))
    target = v[:, None, 0] + a * (v[:, None, 1] - v[:, None, 0]) + b * (v[:, None, 2] - v[:, None, 0])
    d = rng.normal(size=(n, per, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    aimed = np.zeros(n * per, dtype=T.RAY32)
    aimed["origin"] = (target - d * rng.uniform(1.0, 50.0, (n, per, 1))).reshape(-1, 3).astype(np.float32)
    aimed["direction"] = d.reshape(-1, 3).astype(np.float32)
    aimed["t_min"], aimed["t_max"] = 0.001, T.FLT_MAX
    return np.concatenate([row, inc, aimed])


@pytest.mark.parametrize("form", ["LANE", "DUAL_64_2", "LANE8_PERSISTENT_4"])
def test_the_deepest_device_built_tree_is_walked_and_the_next_refused(built, poison, form):
    opts = dict(PLAIN_FORMS.get(form) or PERSISTENT_FORMS[form])
    v, longer = morton_chain(M_ACCEPTED), morton_chain(M_ACCEPTED + 1)
    tris = capi.make_triangles(v)
    rays = morton_rays(v)
    want = po.trace_brute(tris, rays)
    assert (want["prim_id"] >= 0).sum() > 1000 and len(set(want["prim_id"])) > 40
    assert po.OracleScene(v).trace(rays).tobytes() == want.tobytes(), "walk (the host-built tree) == brute force on every ray"
    c = capi.Context(0, **opts)
    try:
        with pytest.raises(capi.MrtError) as e:
            c.build_scene_device(capi.make_triangles(longer))
        assert e.value.status == capi.ERR_UNSUPPORTED and not c.is_available()
        c.build_scene_device(tris)
        assert c.scene_info()["stack_need"] == NEED_ACCEPTED
        for flags in (0, capi.FLAG_COHERENT):
            parity.assert_exact(c.cast(rays, flags=flags), want, f"device-built deep tree {form} flags={flags}: {c.last_kernel_variant()}")
        lit = c.cast(rays, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
        assert np.array_equal(lit.astype(bool), want["prim_id"] >= 0)
        v1 = (v * np.float32(0.5) + np.float32([1.0, -2.0, 0.5])).astype(np.float32)
        tris1 = capi.make_triangles(v1)
        c.refit_scene(tris1)
        assert c.scene_info()["stack_need"] == NEED_ACCEPTED
        rays1 = morton_rays(v1)
        want1 = po.trace_brute(tris1, rays1)
        assert (want1["prim_id"] >= 0).sum() > 1000 and po.OracleScene(v1).trace(rays1).tobytes() == want1.tobytes()
        parity.assert_exact(c.cast(rays1), want1, f"device-built deep tree {form} refit: {c.last_kernel_variant()}")
        findings = lc.check_flat(c.debug_snapshot(), tris1, leaf_boxes="device")
        assert not findings, lc.summary(findings)
    finally:
        c.close()


# ---- record-driven casts share the walk bodies: one family, the shadows ------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 64], ids=lambda n: f"n{n}")
@pytest.mark.parametrize("form", ["LANE", "LANE8_PERSISTENT_4"])
def test_shadow_rays_from_the_grids_records_walk_the_chain(built, poison, form, n):
    opts = dict(PLAIN_FORMS.get(form) or PERSISTENT_FORMS[form])
    inp = inputs(n)
    s = inp["s"]
    rays, hits = inp["sets"]["grid"], inp["want"]["grid"]
    hit = hits["prim_id"] != -1
    pos = rays["origin"] + rays["direction"] * hits["t"][:, None]
    lights = np.zeros(1, dtype=T.LIGHT)
    lights["type"], lights["cast_shadows"], lights["position"] = T.LIGHT_POINT, 1, (n + 2.0, 0.0, 0.0)
    srays, traced = shadow_rays(pos, hits["normal"], hit, lights)
    occluded = po.trace_brute(s["tris"], srays, any_hit=True)["prim_id"] >= 0
    assert np.array_equal(occluded, po.trace(s["wide"], s["leaf_tris"], srays, any_hit=True)["prim_id"] >= 0), "walk == brute on the shadow rays"
    want = (~(traced & occluded)).astype(np.uint8)
    assert want.min() == 0 and want.max() == 1
    c = capi.Context(0, **opts)
    dev = Dev(c)
    try:
        upload_chain(c, n)
        d_rays, d_hits, d_mask = dev.put(rays), dev.put(hits), dev.alloc(rays.shape[0])
        c.cast_shadows(d_rays, d_hits, rays.shape[0], lights, d_mask)
        variant = c.last_kernel_variant()
        assert variant.startswith("trace_shadow_") and ("persistent" in variant) == (form != "LANE"), variant
        np.testing.assert_array_equal(dev.get(d_mask, rays.shape[0], np.uint8), want)
    finally:
        dev.free()
        c.close()
