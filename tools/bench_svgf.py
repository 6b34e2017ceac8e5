"""The SVGF pass chain, timed with device events on the context's stream at 1280x960 and 1920x1080 on a seeded frame (a wall facing the
camera with perturbed normals and positions, 5 % misses, history lengths 1 .. 8 so that 3 pixels in 8 are young; the previous camera
0.37 pixel aside):
  (guides) mrt_svgf_guides from a path state;  (temporal) mrt_svgf_temporal with history;  (variance) mrt_svgf_variance;
  (variance_young) the same with every history length 1: all pixels filtered;  (atrous_N) mrt_svgf_atrous at step N = 1 .. 16;
  (modulate) mrt_svgf_modulate with bytes;  (frame) mrt_svgf_frame with 5 iterations;
  (variance_alt, atrous_N_alt) the same calls of another build of the library (--alt-lib: another form of the two neighbourhood passes,
      built from the revision that holds it or with MRT_EXTRA_DEFINES), in the same process, alternating;
  (copy) a device-to-device copy of one float4 image, 32 bytes per pixel moved: the copy rate every byte floor is taken over.
The variants alternate within every repeat; each timed window is --inner calls back to back.  Prints one line per (size, variant):
median ms per call, the spread, the pass's byte floor (the bytes it must move over the measured copy rate, and over the 6.29 TB/s that
MI355X_MICROARCH.md measured for a float4 copy) and the ratio of its time to that floor; --out writes the same as JSON.  Checked word
for word against numpy (messyerraytracer_amd/svgf.py): temporal and modulate on the whole image, the neighbourhood passes on the
first 64 rows; the alternative build's outputs against this build's.
    python tools/bench_svgf.py [--repeats 20] [--warmup 3] [--inner 20] [--alt-lib PATH] [--quick] [--out profiles/svgf_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, types as T  # noqa: E402
from messyerraytracer_amd import svgf as Sv  # noqa: E402

F = np.float32
HBM_BYTES_PER_S = 6.29e12
# bytes per pixel a pass must move: every input texel read once, every output written once
BYTES = dict(guides=32 + 16 + 32 + 16 + 64, temporal=3 * 16 + 4 * 16 + 2 * 16, variance=4 * 16 + 16, variance_young=4 * 16 + 16, modulate=2 * 16 + 16 + 4,
             frame=(3 * 16 + 4 * 16 + 2 * 16) + (4 * 16 + 16) + 5 * (3 * 16 + 16) + (2 * 16 + 16 + 4), copy=32)
for _s in Sv.STEPS:
    BYTES[f"atrous_{_s}"] = 3 * 16 + 16


class AltLib:
    """the two neighbourhood passes of another build, on a context of its own on the same stream"""

    def __init__(self, path, stream_ptr):
        self.L = C.CDLL(os.path.abspath(path))
        opts = capi.Options()
        opts.struct_size = C.sizeof(capi.Options)
        self.h = C.c_void_p()
        V, U, P = C.c_void_p, C.c_uint32, C.POINTER(Sv.SvgfParams)
        self.L.mrt_create.argtypes = [C.c_int, C.POINTER(capi.Options), C.POINTER(C.c_void_p)]
        self.L.mrt_set_stream.argtypes = [V, V]
        self.L.mrt_destroy.argtypes = [V]
        self.L.mrt_destroy.restype = None
        self.L.mrt_svgf_variance.argtypes = [V, P, U, U, V, V, V, V, V, U]
        self.L.mrt_svgf_atrous.argtypes = [V, P, U, U, U, V, V, V, V, U]
        assert self.L.mrt_create(0, C.byref(opts), C.byref(self.h)) == 0
        assert self.L.mrt_set_stream(self.h, C.c_void_p(stream_ptr)) == 0

    def variance(self, p, w, h, illum, moments, nd, pos, out):
        assert self.L.mrt_svgf_variance(self.h, C.byref(p), w, h, illum, moments, nd, pos, out, capi.FLAG_ASYNC) == 0

    def atrous(self, p, w, h, step, illum, nd, pos, out):
        assert self.L.mrt_svgf_atrous(self.h, C.byref(p), w, h, step, illum, nd, pos, out, capi.FLAG_ASYNC) == 0

    def close(self):
        self.L.mrt_destroy(self.h)


def look_basis():
    return np.eye(3, dtype=F)   # x right, y up, the camera looks along -z


def wall(cam, w, h, rng):
    """(normal_depth, position) of the plane z = 0 seen by cam, normals and positions perturbed, 5 % misses"""
    ys, xs = np.mgrid[0:h, 0:w]
    u = (F(2) * (xs.astype(F) + F(cam.jitter_x)) * F(cam.inv_w)) - F(1)
    v = F(1) - (F(2) * (ys.astype(F) + F(cam.jitter_y)) * F(cam.inv_h))
    r, up, f, o = (np.array(list(a), F) for a in (cam.right, cam.up, cam.fwd, cam.origin))
    d = r * (u * F(cam.half_w))[..., None] + up * (v * F(cam.half_h))[..., None] - f
    d = (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(F)
    t = (-o[2] / d[..., 2]).astype(F)
    nd, pos = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    n = np.array([0, 0, 1], F) + 0.02 * rng.normal(0, 1, (h, w, 3))
    nd[..., :3], nd[..., 3] = (n / np.linalg.norm(n, axis=2, keepdims=True)), t
    pos[..., :3] = o + d * t[..., None]
    pos[..., 2] += (0.006 * rng.uniform(-1, 1, (h, w))).astype(F)
    miss = rng.uniform(0, 1, (h, w)) < 0.05
    nd[miss], pos[miss] = 0, 0
    return nd, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = ((1280, 960), (1920, 1080))
    if a.quick:
        sizes, a.repeats, a.warmup, a.inner = ((160, 96),), 2, 1, 2
    stream = torch.cuda.Stream()  # a stream of its own: the default stream's handle is null, which mrt_set_stream reads as "the context's own"
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    alt = AltLib(a.alt_lib, stream.cuda_stream) if a.alt_lib else None
    ok, results = True, []
    A = capi.FLAG_ASYNC
    for w, h in sizes:
        n = w * h
        rng = np.random.default_rng(11)
        cam = capi.ray_camera((0.0, 0.0, 3.0), look_basis(), w, h, 40.0)
        foot = 2.0 * cam.half_w * 3.0 / w
        prev_cam = capi.ray_camera((-0.37 * foot, 0.37 * foot, 3.0), look_basis(), w, h, 40.0)
        host = {}
        host["nd"], host["pos"] = wall(cam, w, h, rng)
        host["prev_nd"], host["prev_pos"] = wall(prev_cam, w, h, rng)
        for k in ("illum", "prev_illum"):
            host[k] = rng.uniform(0, 1, (h, w, 4)).astype(F)
            host[k][..., 3] = rng.uniform(0.01, 0.05, (h, w))
        for k in ("moments", "prev_moments"):
            m1 = rng.uniform(0, 1, (h, w))
            host[k] = np.stack([m1, m1 * m1 + rng.uniform(0, 0.05, (h, w)), rng.integers(1, 9, (h, w)), np.zeros((h, w))], axis=2).astype(F)
        host["moments_young"] = host["moments"].copy()
        host["moments_young"][..., 2] = 1
        host["albedo"] = np.concatenate([rng.uniform(0.05, 1, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(F)
        rays, hits, rows, state = np.zeros(n, T.RAY32), np.zeros(n, T.HIT32), np.zeros(n, T.SURFACE64), np.zeros(n, T.PATH_STATE)
        rays["origin"], rays["direction"] = rng.uniform(-3, 3, (n, 3)), rng.normal(0, 1, (n, 3))
        hits["t"], hits["prim_id"] = rng.uniform(0.1, 40, n), rng.integers(-1, 3, n)
        rows["normal"], rows["albedo"], state["radiance"] = rng.normal(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3)), rng.uniform(0, 4, (n, 3))
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        for k, v in dict(rays=rays, hits=hits, rows=rows, state=state).items():
            dev[k] = torch.from_numpy(v.view(np.uint8)).cuda()
        outs = ("g_illum", "g_albedo", "g_nd", "g_pos", "t_illum", "t_moments", "var", "var_young", "var_alt", "rgba", "f_illum", "f_moments", "f_a", "f_b", "f_rgba",
                "c_dst") + tuple(f"a{s}" for s in Sv.STEPS) + tuple(f"a{s}_alt" for s in Sv.STEPS)
        for k in outs:
            dev[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        dev["rgba8"] = torch.empty(n, dtype=torch.int32, device="cuda")
        ptr = {k: v.data_ptr() for k, v in dev.items()}
        p = Sv.params(has_history=True, tonemap_mode=3)
        prev4 = (ptr["prev_illum"], ptr["prev_moments"], ptr["prev_nd"], ptr["prev_pos"])
        fns = {
            "guides": lambda: Sv.svgf_guides(ctx, ptr["rays"], ptr["hits"], ptr["rows"], Sv.SRC_PATH_STATE, ptr["state"], n, ptr["g_illum"], ptr["g_albedo"],
                                             ptr["g_nd"], ptr["g_pos"], flags=A),
            "temporal": lambda: Sv.svgf_temporal(ctx, p, w, h, ptr["illum"], ptr["nd"], ptr["pos"], prev_cam, *prev4, ptr["t_illum"], ptr["t_moments"], flags=A),
            "variance": lambda: Sv.svgf_variance(ctx, p, w, h, ptr["illum"], ptr["moments"], ptr["nd"], ptr["pos"], ptr["var"], flags=A),
            "variance_young": lambda: Sv.svgf_variance(ctx, p, w, h, ptr["illum"], ptr["moments_young"], ptr["nd"], ptr["pos"], ptr["var_young"], flags=A),
        }
        if alt:
            fns["variance_alt"] = lambda: alt.variance(p, w, h, ptr["illum"], ptr["moments"], ptr["nd"], ptr["pos"], ptr["var_alt"])
        for s in Sv.STEPS:
            fns[f"atrous_{s}"] = lambda s=s: Sv.svgf_atrous(ctx, p, w, h, s, ptr["illum"], ptr["nd"], ptr["pos"], ptr[f"a{s}"], flags=A)
            if alt:
                fns[f"atrous_{s}_alt"] = lambda s=s: alt.atrous(p, w, h, s, ptr["illum"], ptr["nd"], ptr["pos"], ptr[f"a{s}_alt"])
        fns["modulate"] = lambda: Sv.svgf_modulate(ctx, p, w, h, ptr["illum"], ptr["albedo"], ptr["rgba"], ptr["rgba8"], flags=A)
        fns["frame"] = lambda: Sv.svgf_frame(ctx, p, w, h, ptr["illum"], ptr["albedo"], ptr["nd"], ptr["pos"], prev_cam, *prev4, ptr["f_illum"], ptr["f_moments"],
                                             ptr["f_a"], ptr["f_b"], ptr["f_rgba"], None, flags=A)
        fns["copy"] = lambda: dev["c_dst"].copy_(dev["illum"])
        # what is computed, once
        for fn in fns.values():
            fn()
        ctx.synchronize()
        stream.synchronize()
        rows_c = min(h, 64)

        def crop(k, reach):
            return host[k][:min(h, rows_c + reach)]

        def equal(k, want, top=None):
            got = dev[k].cpu().numpy()
            got, want = (got, want) if top is None else (got[:top], want[:top])
            return bool(np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)))

        same = True
        ti, tm = Sv.temporal(p, host["illum"], host["nd"], host["pos"], prev_cam, host["prev_illum"], host["prev_moments"], host["prev_nd"], host["prev_pos"])
        same &= equal("t_illum", ti) and equal("t_moments", tm)
        same &= equal("rgba", Sv.modulate(p, host["illum"], host["albedo"]))
        same &= equal("var", Sv.variance(p, crop("illum", 3), crop("moments", 3), crop("nd", 3), crop("pos", 3)), rows_c)
        same &= equal("var_young", Sv.variance(p, crop("illum", 3), crop("moments_young", 3), crop("nd", 3), crop("pos", 3)), rows_c)
        for s in Sv.STEPS:
            same &= equal(f"a{s}", Sv.atrous(p, s, crop("illum", 2 * s), crop("nd", 2 * s), crop("pos", 2 * s)), rows_c)
            if alt:
                same &= bool(torch.equal(dev[f"a{s}"].view(torch.int32), dev[f"a{s}_alt"].view(torch.int32)))
        if alt:
            same &= bool(torch.equal(dev["var"].view(torch.int32), dev["var_alt"].view(torch.int32)))
        gi = Sv.guides(rays, hits, rows, state["radiance"])
        for k, wnt in zip(("g_illum", "g_albedo", "g_nd", "g_pos"), gi):
            same &= equal(k, wnt.reshape(h, w, 4))
        ok &= bool(same)
        young = float(((host["moments"][..., 2] < 4) & (host["nd"][..., 3] > 0)).mean())

        times = {v: [] for v in fns}
        for rep in range(a.warmup + a.repeats):
            for v, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.inner):
                    fn()
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    times[v].append(e0.elapsed_time(e1) / a.inner)
        med = {v: float(np.median(t)) for v, t in times.items()}
        rate = n * BYTES["copy"] / (med["copy"] * 1e-3)
        print(f"{w}x{h} equal to numpy: {bool(same)}; young pixels {young:.3f}; measured copy rate {rate / 1e12:.2f} TB/s", flush=True)
        for v, t in times.items():
            b = BYTES[v[:-4] if v.endswith("_alt") else v]
            floor, floor_doc = n * b / rate * 1e3, n * b / HBM_BYTES_PER_S * 1e3
            results.append(dict(size=f"{w}x{h}", pixels=n, variant=v, median_ms=med[v], min_ms=min(t), max_ms=max(t), windows=len(t), calls_per_window=a.inner,
                                bytes_per_pixel=b, floor_ms=floor, floor_ms_at_6_29=floor_doc, ratio=med[v] / floor))
            print(f"{w}x{h} ({v:15s}) {med[v]:9.4f} ms  [{min(t):.4f} .. {max(t):.4f}] n={len(t)} x {a.inner}  {b:4d} B/pixel  floor {floor:.4f} ms "
                  f"({floor_doc:.4f} at 6.29 TB/s)  {med[v] / floor:7.1f}x", flush=True)
        del dev
    if alt:
        alt.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_svgf.py", equal=bool(ok), alt_lib=bool(a.alt_lib), rows=results), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
