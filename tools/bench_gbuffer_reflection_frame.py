"""The reflection pass of a hybrid frame on synth.room(), flat and as a two-level scene: one closest-hit mirror ray per pixel, made
either from a rasteriser's depth and normal-roughness buffers or from the primary grid's resident hit records, on the same surfaces in
one session, timed with device events on the context's stream:
  (g) mrt_cast_gbuffer_reflections: the G-buffer of the primary grid's hits (depths projected in float64 through the camera of
      messyerraytracer_amd/gbuffer.py fitted to the grid's, normals octahedral-encoded, one roughness below the threshold everywhere);
  (r) mrt_cast_grid_reflections on the records themselves;
  (i) mrt_reflection_image of (g)'s records, on its own.
The variants alternate within every repeat.  Prints one line per (scene, size, variant): median ms per pass and the spread (min ..
max) over the repeats, plus the kernel the library chose.  Checked: (g)'s rays equal the numpy restatement byte for byte, its records
equal mrt_cast of the restated rays, (i) equals the restated image; and, for information, how many pixels reflect onto the same
triangle in (g) and (r) (the two differ by the rounding of the reconstructed position and of the encoded normal).
    python tools/bench_gbuffer_reflection_frame.py [--repeats 20] [--warmup 5] [--quick]
--quick: the flat scene at one size, few repeats."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import gbuffer as G  # noqa: E402

F = np.float32
CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
MAX_DIST = F(25.0)
NEAR, FAR = 0.1, 100.0
ROUGHNESS, THRESHOLD = F(0.1), F(0.3)


def fitted_camera(w, h):
    """gbuffer.Camera through the grid's pixel centres: the library's field of view is horizontal"""
    fov_y = np.degrees(2 * np.arctan(np.tan(np.radians(CAM[2]) / 2) / (w / h)))
    return G.Camera(CAM[0], np.add(CAM[0], CAM[1]), fov_y=fov_y, aspect=w / h, near=NEAR, far=FAR)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes, kinds = ((1280, 960), (1920, 1080)), ("flat", "two-level")
    if a.quick:
        sizes, kinds, a.repeats, a.warmup = ((1280, 960),), ("flat",), 5, 2
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    stream = torch.cuda.current_stream()
    ok = True
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    for kind in kinds:
        ctx = capi.Context(0)
        ctx.set_stream(stream.cuda_stream)
        if kind == "flat":
            tris = capi.make_triangles(verts, layers=layers)
            nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts))
            ctx.upload_scene(tris, nodes, prim_idx)
        else:
            ctx.upload_two_level_scene(local, inst)
        for w, h in sizes:
            n = w * h
            cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
            d_prim = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            ctx.generate_grid(cam, w, h, 0, h, d_prim)
            rays = d_prim.cpu().numpy().view(T.RAY32)
            d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
            hits = d_hits.cpu().numpy().view(T.HIT32)
            # the G-buffer of those hits
            gcam = fitted_camera(w, h)
            fit = float(np.abs(gcam.primary_rays(w, h)["direction"] - rays["direction"]).max())
            hit = hits["prim_id"] != -1
            points = rays["origin"].astype(np.float64) + rays["direction"].astype(np.float64) * hits["t"].astype(np.float64)[:, None]
            with np.errstate(invalid="ignore", over="ignore"):
                depth = np.where(hit, gcam.depth(points), 1.0).astype(F)
            guide = np.zeros((n, 4), F)
            guide[:, :2] = G.octahedral_encode(np.where(hit[:, None], hits["normal"], (0.0, 0.0, 1.0)))
            guide[:, 2] = ROUGHNESS
            g = G.GBuffer(depth, guide, gcam.inv_projection, gcam.inv_view, G.NORMAL_OCTAHEDRAL, THRESHOLD, MAX_DIST)
            d_depth, d_guide = dev(depth), dev(guide)
            desc = g.desc(d_depth.data_ptr(), d_guide.data_ptr())
            d_out_g, d_rays_g = (torch.empty(n * 32, dtype=torch.uint8, device="cuda") for _ in range(2))
            d_out_r = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            d_img = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
            kernels = {}

            def run_g():
                G.cast_gbuffer_reflections(ctx, desc, w, h, d_out_g.data_ptr())
                kernels["g"] = ctx.last_kernel_variant()

            def run_r():
                ctx.cast_grid_reflections(cam, w, h, d_hits, d_out_r, MAX_DIST)
                kernels["r"] = ctx.last_kernel_variant()

            def run_i():
                G.reflection_image_device(ctx, desc, w, h, d_out_g.data_ptr(), d_img.data_ptr())
                kernels["i"] = "reflection_image_kernel"

            times = {"g": [], "r": [], "i": []}
            for rep in range(a.warmup + a.repeats):
                for name, fn in (("g", run_g), ("r", run_r), ("i", run_i)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        times[name].append(e0.elapsed_time(e1))
            # the outputs: rays against the restatement, records against mrt_cast of the restated rays, the image against the restatement
            G.cast_gbuffer_reflections(ctx, desc, w, h, d_out_g.data_ptr(), d_rays_g.data_ptr())
            want_rays, traced = G.gbuffer_rays(g, w, h)
            got_hits = d_out_g.cpu().numpy().view(T.HIT32)
            rays_ok = np.array_equal(d_rays_g.cpu().numpy(), want_rays.view(np.uint8))
            recast = ctx.cast(want_rays)
            hits_ok = np.array_equal(got_hits.view(np.uint8), recast.view(np.uint8))
            img_ok = np.array_equal(d_img.cpu().numpy().view(np.uint32), G.reflection_image(g, w, h, got_hits).view(np.uint32).reshape(-1))
            same = rays_ok and hits_ok and img_ok
            ok &= same
            rec = d_out_r.cpu().numpy().view(T.HIT32)
            agree = float((rec["prim_id"] == got_hits["prim_id"]).mean())
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, label in (("g", "mrt_cast_gbuffer_reflections"), ("r", "mrt_cast_grid_reflections"), ("i", "mrt_reflection_image")):
                v = times[k]
                print(f"{kind} {w}x{h} rays={n} ({k}) {label:30s} {med[k]:8.3f} ms  [{min(v):.3f} .. {max(v):.3f}]  {kernels[k]}", flush=True)
            print(f"{kind} {w}x{h} rays / records / image equal the restatement: {rays_ok} / {hits_ok} / {img_ok}; traced {float(traced.mean()):.3f}; "
                  f"reflected hits {float((got_hits['prim_id'] != -1).mean()):.3f}; same triangle as (r) in {agree:.4f} of the pixels; "
                  f"camera fit {fit:.2e}; (g) / (r) = {med['g'] / med['r']:.2f}; (i) / (g) = {med['i'] / med['g']:.2f}", flush=True)
        ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
