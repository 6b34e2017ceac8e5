"""The bounce pass of a path tracer's frame on synth.room(), flat and as a two-level scene: from the primary grid's resident hit
records and a per-record {metallic, roughness} array (metallic cycling 0, 0.5, 1, roughness 0.02, 0.3, 1), one bounce ray per pixel
(closest-hit, t_max = 1e30), three ways of producing the same records, timed with device events on the context's stream:
  (a) the host round trip: download the records, sample the rays in numpy (messyerraytracer_amd/bounce.py), mrt_cast from host arrays;
  (b) device-resident rays (sampled on the host once, untimed) cast with mrt_cast(RAYS/HITS_ON_DEVICE) -- Morton keys, sort and
      gather included;
  (c) mrt_cast_grid_bounce.
The variants alternate within every repeat; (a), which takes a large fraction of a second, runs in the first --host-repeats timed
repeats only.  Prints one line per (scene, size, variant): median ms per pass and the spread (min .. max) over the repeats, plus the
kernel the library chose; every output is checked byte-equal across (a), (b) and (c).
    python tools/bench_bounce_frame.py [--repeats 20] [--warmup 5] [--host-repeats 3] [--quick]
--quick: the flat scene at one size, few repeats (for a kernel-trace run under rocprofv3)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import bounce as B  # noqa: E402

F = np.float32
CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
FRAME, FIRST_DRAW, T_MAX = 1, 0, F(1e30)
METALLIC, ROUGHNESS = np.array([0.0, 0.5, 1.0], F), np.array([0.02, 0.3, 1.0], F)


def surface(n):
    i = np.arange(n)
    return np.stack([METALLIC[i % 3], ROUGHNESS[(i // 3) % 3]], axis=1).astype(F)


def host_rays(rays, hits, surf):
    """The sampler of include/mrt_hip.h in numpy float32 (the reference's placeholder ray where an entry has no ray)."""
    with np.errstate(over="ignore", invalid="ignore"):
        pos = rays["origin"] + rays["direction"] * hits["t"][:, None]
    out, _, lobe = B.bounce_rays(rays["direction"], pos, hits["normal"], hits["prim_id"] != -1, np.arange(rays.shape[0]), FRAME,
                                 FIRST_DRAW, T_MAX, surf[:, 0], surf[:, 1])
    return out, lobe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes, kinds = ((1280, 960), (1920, 1080)), ("flat", "two-level")
    if a.quick:
        sizes, kinds, a.repeats, a.warmup, a.host_repeats = ((1280, 960),), ("flat",), 5, 2, 1
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    stream = torch.cuda.current_stream()
    ok = True
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
            ctx.generate_grid(cam, w, h, 0, h, d_prim)   # the primary rays the grid cast traces, for (a) and (b)
            rays = d_prim.cpu().numpy().view(T.RAY32)
            d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
            surf = surface(n)
            d_surf = torch.from_numpy(surf.view(np.uint8).reshape(-1)).cuda()
            rays_b, lobe_b = host_rays(rays, d_hits.cpu().numpy().view(T.HIT32), surf)
            d_rays_b = torch.from_numpy(rays_b.view(np.uint8)).cuda()
            d_out_b = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            d_out_c = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            d_lobe_c = torch.empty(n, dtype=torch.uint8, device="cuda")
            out = {}

            def run_a():
                hits = d_hits.cpu().numpy().view(T.HIT32)  # download (on the stream, then the host waits)
                out["a"] = ctx.cast(host_rays(rays, hits, surf)[0], mode=capi.MODE_NEAREST)

            def run_b():
                ctx.cast(d_rays_b, d_out_b, count=n, mode=capi.MODE_NEAREST, flags=capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE)
                out["b"], out["b_kernel"] = d_out_b, ctx.last_kernel_variant()

            def run_c():
                ctx.cast_grid_bounce(cam, w, h, d_hits, d_out_c, frame=FRAME, first_draw=FIRST_DRAW, t_max=T_MAX, d_surface=d_surf,
                                     d_out_lobe=d_lobe_c)
                out["c"], out["c_kernel"] = d_out_c, ctx.last_kernel_variant()

            times = {"a": [], "b": [], "c": []}
            for rep in range(a.warmup + a.repeats):
                for v, fn in (("a", run_a), ("b", run_b), ("c", run_c)):
                    if v == "a" and not (rep == 0 or a.warmup <= rep < a.warmup + a.host_repeats):
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        times[v].append(e0.elapsed_time(e1))
            ra = np.ascontiguousarray(out["a"]).view(np.uint8)
            rb, rc = out["b"].cpu().numpy(), out["c"].cpu().numpy()
            lobe_c = d_lobe_c.cpu().numpy()
            same = np.array_equal(ra, rb) and np.array_equal(ra, rc) and np.array_equal(lobe_c, lobe_b)
            ok &= same
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, label in (("a", "host round trip"), ("b", "device rays + mrt_cast"), ("c", "mrt_cast_grid_bounce")):
                v = times[k]
                print(f"{kind} {w}x{h} bounce rays={n} ({k}) {label:26s} {med[k]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}"
                      + (f"  {out[k + '_kernel']}" if k != "a" else ""), flush=True)
            print(f"{kind} {w}x{h} bounce outputs byte-equal: {same}; lobes none/diffuse/specular "
                  f"{[round(float((lobe_c == x).mean()), 3) for x in (0, 1, 2)]}; bounce hits {float((out['a']['prim_id'] != -1).mean()):.3f}; "
                  f"(c) not slower than (b): {med['c'] <= med['b']} ({med['b'] / med['c']:.2f}x), than (a): {med['a'] / med['c']:.0f}x",
                  flush=True)
            del d_rays_b, d_out_b, d_out_c, d_lobe_c, d_surf
        ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
