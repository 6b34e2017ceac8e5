"""The reflection pass of a renderer's frame on synth.room(), flat and as a two-level scene: one closest-hit mirror ray per pixel from the
primary grid's resident hit records, three ways of producing the same records, timed with device events on the context's stream:
  (a) the host round trip: download the records, build the rays in numpy, mrt_cast(NEAREST) from host arrays;
  (b) device-resident rays (built on the host once, untimed) cast with mrt_cast(NEAREST, RAYS/HITS_ON_DEVICE) -- Morton keys, sort and
      gather included;
  (c) mrt_cast_grid_reflections.
The variants alternate within every repeat.  Prints one line per (scene, size, variant): median ms per reflection pass and the spread
(min .. max) over the repeats, plus the kernel the library chose; every output is checked byte-equal across (a), (b) and (c).
    python tools/bench_reflection_frame.py [--repeats 20] [--warmup 5] [--quick]
--quick: the flat scene at one size, few repeats (for a kernel-trace run under rocprofv3)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402

F = np.float32
CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
MAX_DIST = F(25.0)


def host_rays(rays, hits):
    """The formula of include/mrt_hip.h in numpy float32 (the reference's placeholder ray where a record has no ray)."""
    with np.errstate(over="ignore", invalid="ignore"):
        hit = hits["prim_id"] != -1
        d = rays["direction"]
        pos = rays["origin"] + d * hits["t"][:, None]
        n = hits["normal"].copy()
        c = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        n[c > F(0)] = -n[c > F(0)]
        k = F(2) * ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2])
        out = np.zeros(rays.shape[0], dtype=T.RAY32)
        out["direction"] = d - k[:, None] * n
        out["origin"] = pos + n * F(0.01)
        out["t_max"] = MAX_DIST
        out[~hit] = np.array([((0, 0, 0), 0, (0, 1, 0), 0)], dtype=T.RAY32)[0]
    return out


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
            d_rays_b = torch.from_numpy(host_rays(rays, d_hits.cpu().numpy().view(T.HIT32)).view(np.uint8)).cuda()
            d_out_b = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            d_out_c = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            out = {}

            def run_a():
                hits = d_hits.cpu().numpy().view(T.HIT32)  # download (on the stream, then the host waits)
                out["a"] = ctx.cast(host_rays(rays, hits))

            def run_b():
                ctx.cast(d_rays_b, d_out_b, count=n, flags=capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE)
                out["b"] = d_out_b

            def run_c():
                ctx.cast_grid_reflections(cam, w, h, d_hits, d_out_c, MAX_DIST)
                out["c"] = d_out_c
                out["c_kernel"] = ctx.last_kernel_variant()

            times = {"a": [], "b": [], "c": []}
            for rep in range(a.warmup + a.repeats):
                for name, fn in (("a", run_a), ("b", run_b), ("c", run_c)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        times[name].append(e0.elapsed_time(e1))
            ra = out["a"].view(np.uint8)
            same = np.array_equal(ra, out["b"].cpu().numpy()) and np.array_equal(ra, out["c"].cpu().numpy())
            ok &= same
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, label in (("a", "host round trip"), ("b", "device rays + mrt_cast"), ("c", "mrt_cast_grid_reflections")):
                v = times[k]
                print(f"{kind} {w}x{h} rays={n} ({k}) {label:26s} {med[k]:8.3f} ms  [{min(v):.3f} .. {max(v):.3f}]"
                      + (f"  {out['c_kernel']}" if k == "c" else ""), flush=True)
            hit = out["a"]["prim_id"] != -1
            print(f"{kind} {w}x{h} outputs byte-equal: {same}; reflected hits {float(hit.mean()):.3f}; "
                  f"(c) faster than (b): {med['c'] < med['b']} ({med['b'] / med['c']:.2f}x), than (a): {med['a'] / med['c']:.1f}x", flush=True)
        ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
