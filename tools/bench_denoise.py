"""The reflection effect's image passes, timed with device events on the context's stream at 1280x960 and 1920x1080 (Godot's octahedral
normals, seeded images, history present), for r = 2 and r = 4:
  (spatial) mrt_denoise_spatial, the form this tree keeps;
  (spatial_alt) the same call of another build of the library (--alt-lib: the other form of the spatial pass, built from the revision
      that holds it or with MRT_EXTRA_DEFINES), in the same process, alternating -- plain against tiled;
  (three) mrt_denoise_spatial -> mrt_denoise_temporal in place -> mrt_composite_reflections;
  (fused) mrt_resolve_reflections without d_denoised;
  (copy) a device-to-device copy of the fused call's bytes -- per pixel 16 (reflection) + 4 (depth) + 16 (guide) read, 16 + 16 (history,
      colour) read and written: 100 bytes, 50 copied -- the byte floor measured in the same run; the floor is also printed over the
      6.29 TB/s that MI355X_MICROARCH.md measured for a float4 copy.
The variants alternate within every repeat; each timed window is --inner calls back to back.  Prints one line per (size, radius,
variant): median ms per call and the spread; --out writes the same as JSON.  Checked word for word against numpy
(messyerraytracer_amd/denoise.py): the first 64 rows of the denoised image and of both histories, the whole colour of both paths (from
the device's history); the two histories against each other, and the alternative build's output against this build's.
    python tools/bench_denoise.py [--repeats 20] [--warmup 3] [--inner 50] [--alt-lib PATH] [--quick] [--out profiles/denoise_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi  # noqa: E402
from messyerraytracer_amd import denoise as Dn  # noqa: E402

F = np.float32
FUSED_BYTES = 100
HBM_BYTES_PER_S = 6.29e12


class AltLib:
    """mrt_denoise_spatial of another build, on a context of its own on the same stream"""

    def __init__(self, path, stream_ptr):
        self.L = C.CDLL(os.path.abspath(path))
        opts = capi.Options()
        opts.struct_size = C.sizeof(capi.Options)
        self.h = C.c_void_p()
        V, U = C.c_void_p, C.c_uint32
        self.L.mrt_create.argtypes = [C.c_int, C.POINTER(capi.Options), C.POINTER(C.c_void_p)]
        self.L.mrt_set_stream.argtypes = [V, V]
        self.L.mrt_destroy.argtypes = [V]
        self.L.mrt_destroy.restype = None
        self.L.mrt_denoise_spatial.argtypes = [V, C.POINTER(Dn.DenoiseParams), U, U, V, V, V, V, U]
        assert self.L.mrt_create(0, C.byref(opts), C.byref(self.h)) == 0
        assert self.L.mrt_set_stream(self.h, C.c_void_p(stream_ptr)) == 0

    def spatial(self, p, w, h, refl, depth, guide, out):
        rc = self.L.mrt_denoise_spatial(self.h, C.byref(p), w, h, refl, depth, guide, out, capi.FLAG_ASYNC)
        assert rc == 0, rc

    def close(self):
        self.L.mrt_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes, radii = ((1280, 960), (1920, 1080)), (2, 4)
    if a.quick:
        sizes, a.repeats, a.warmup, a.inner = ((160, 96),), 2, 1, 2
    stream = torch.cuda.Stream()  # a stream of its own: the default stream's handle is null, which mrt_set_stream reads as "the context's own"
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    alt = AltLib(a.alt_lib, stream.cuda_stream) if a.alt_lib else None
    ok, results = True, []
    for w, h in sizes:
        n = w * h
        rng = np.random.default_rng(11)
        refl = rng.uniform(0, 1, (h, w, 4)).astype(F)
        refl[..., 3] = np.where(rng.uniform(0, 1, (h, w)) < 0.1, 0, refl[..., 3])
        depth = rng.uniform(0, 0.99, (h, w)).astype(F)
        guide = rng.uniform(0, 1, (h, w, 4)).astype(F)
        guide[..., :2] = (0.5 + 0.1 * rng.normal(0, 1, (h, w, 2))).clip(0, 1)
        hist = rng.uniform(0, 1, (h, w, 4)).astype(F)
        color = rng.uniform(0, 1, (h, w, 4)).astype(F)
        dev = {k: torch.from_numpy(v).cuda() for k, v in dict(refl=refl, depth=depth, guide=guide, hist=hist, color=color).items()}
        for k in ("den", "den_alt", "hist3", "color3", "histf", "colorf"):
            dev[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        c_src, c_dst = torch.empty(n * FUSED_BYTES // 2, dtype=torch.uint8, device="cuda"), torch.empty(n * FUSED_BYTES // 2, dtype=torch.uint8, device="cuda")
        ptr = {k: v.data_ptr() for k, v in dev.items()}
        for radius in radii:
            p = Dn.params(normal_kind=Dn.NORMAL_OCTAHEDRAL, has_history=True, kernel_radius=radius)
            A = capi.FLAG_ASYNC

            def spatial():
                Dn.denoise_spatial(ctx, p, w, h, ptr["refl"], ptr["depth"], ptr["guide"], ptr["den"], flags=A)

            def spatial_alt():
                alt.spatial(p, w, h, ptr["refl"], ptr["depth"], ptr["guide"], ptr["den_alt"])

            def three():
                Dn.denoise_spatial(ctx, p, w, h, ptr["refl"], ptr["depth"], ptr["guide"], ptr["den"], flags=A)
                Dn.denoise_temporal(ctx, p, w, h, ptr["den"], ptr["hist3"], ptr["hist3"], flags=A)
                Dn.composite_reflections(ctx, p, w, h, ptr["hist3"], ptr["depth"], ptr["guide"], ptr["color3"], flags=A)

            def fused():
                Dn.resolve_reflections(ctx, p, w, h, ptr["refl"], ptr["depth"], ptr["guide"], ptr["histf"], ptr["colorf"], flags=A)

            def copy():
                c_dst.copy_(c_src)

            # what is computed, once, on fresh history and colour
            for k in ("hist3", "histf"):
                dev[k].copy_(dev["hist"])
            for k in ("color3", "colorf"):
                dev[k].copy_(dev["color"])
            three()
            fused()
            if alt:
                spatial_alt()
            ctx.synchronize()
            stream.synchronize()
            rows, taps = min(h, 64), min(h, 68)                                          # (the four rows below the first 64 are only taps)
            want_den = Dn.spatial(p, refl[:taps], depth[:taps], guide[:taps])
            want_hist = Dn.temporal(p, want_den, hist[:taps])
            got_hist = dev["hist3"].cpu().numpy()
            want_color = Dn.composite(p, got_hist, depth, guide, color)                  # per pixel: the whole image, from the device's history
            same = True
            for k, wnt in (("den", want_den), ("hist3", want_hist), ("histf", want_hist)):
                same &= np.array_equal(dev[k][:rows].cpu().numpy().view(np.uint32), wnt[:rows].view(np.uint32))
            for k in ("color3", "colorf"):
                same &= np.array_equal(dev[k].cpu().numpy().view(np.uint32), want_color.view(np.uint32))
            same &= bool(torch.equal(dev["hist3"].view(torch.int32), dev["histf"].view(torch.int32)))
            if alt:
                same &= bool(torch.equal(dev["den"].view(torch.int32), dev["den_alt"].view(torch.int32)))
            ok &= bool(same)

            variants = [("spatial", spatial)] + ([("spatial_alt", spatial_alt)] if alt else []) + [("three", three), ("fused", fused), ("copy", copy)]
            times = {v: [] for v, _ in variants}
            for rep in range(a.warmup + a.repeats):
                for v, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.inner):
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        times[v].append(e0.elapsed_time(e1) / a.inner)
            m = {}
            for v, _ in variants:
                t = times[v]
                m[v] = float(np.median(t))
                results.append(dict(size=f"{w}x{h}", pixels=n, radius=radius, variant=v, median_ms=m[v], min_ms=min(t), max_ms=max(t), windows=len(t),
                                    calls_per_window=a.inner))
                print(f"{w}x{h} r={radius} ({v}) {m[v]:9.4f} ms  [{min(t):.4f} .. {max(t):.4f}] n={len(t)} x {a.inner}", flush=True)
            floor = n * FUSED_BYTES / HBM_BYTES_PER_S * 1e3
            line = f"{w}x{h} r={radius} equal to numpy: {bool(same)}; fused / three: {m['fused'] / m['three']:.3f}x; fused / copy: {m['fused'] / m['copy']:.2f}x; "
            line += f"byte floor {floor:.4f} ms ({FUSED_BYTES} B/pixel at 6.29 TB/s): fused is {m['fused'] / floor:.1f}x it"
            if alt:
                line += f"; spatial / spatial_alt: {m['spatial'] / m['spatial_alt']:.3f}x"
            print(line, flush=True)
        del dev, c_src, c_dst
    if alt:
        alt.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/bench_denoise.py", equal=bool(ok), alt_lib=bool(a.alt_lib), rows=results), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
