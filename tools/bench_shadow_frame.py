"""The shadow pass of a renderer's frame on synth.room(): one any-hit ray per (pixel, light) from the primary grid's resident hit
records, three ways of producing the same lit mask, timed with device events on the context's stream:
  (a) the reference's host round trip: download the records, build the rays in numpy, mrt_cast from host arrays, invert;
  (b) device-resident rays (built on the host once, untimed) cast with mrt_cast(ANY_HIT, BOOL_OUT, RAYS/HITS_ON_DEVICE) --
      Morton keys, sort and gather included -- and inverted on the device;
  (c) mrt_cast_grid_shadows.
The variants alternate within every repeat.  Prints one line per (size, lights, variant): median ms per shadow pass and the spread
(min .. max) over the repeats, plus the kernel the library chose; every output is checked byte-equal across (a), (b) and (c).
    python tools/bench_shadow_frame.py [--repeats 20] [--warmup 5] [--quick]
--quick: one size, one light count, few repeats (for a kernel-trace run under rocprofv3)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402

F = np.float32
CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)


def lights(n):
    L = np.zeros(4, dtype=T.LIGHT)
    L["cast_shadows"] = 1
    L[0]["type"], L[0]["position"] = T.LIGHT_POINT, (1.0, 4.5, 1.5)
    L[1]["type"], L[1]["direction"] = T.LIGHT_DIRECTIONAL, (0.3, 1.0, 0.2)
    L[2]["type"], L[2]["position"] = T.LIGHT_SPOT, (-3.0, 5.0, -3.0)
    L[3]["type"], L[3]["position"] = T.LIGHT_POINT, (3.5, 2.0, 3.5)
    return L[:n].copy()


def host_rays(rays, hits, ls):
    """The formula of include/mrt_hip.h in numpy float32: rays of every pair (the reference's degenerate ray where it traces none)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        hit = hits["prim_id"] != -1
        org = (rays["origin"] + rays["direction"] * hits["t"][:, None]) + hits["normal"] * F(1e-3)
        out = np.zeros((len(ls), rays.shape[0]), dtype=T.RAY32)
        for l, L in enumerate(ls):
            r = out[l]
            r["origin"] = org
            if L["type"] == T.LIGHT_DIRECTIONAL:
                r["direction"], r["t_max"], ok = L["direction"].astype(F), F(1000.0), hit
            else:
                to = L["position"].astype(F)[None, :] - org
                dist = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2])
                r["direction"], r["t_max"], ok = to / dist[:, None], dist, hit & ~(dist < F(1e-6))
            r[~ok] = np.array([((0, 0, 0), 0, (0, 1, 0), 0)], dtype=T.RAY32)[0]
    return out.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes, counts = ((1280, 960), (1920, 1080)), (1, 4)
    if a.quick:
        sizes, counts, a.repeats, a.warmup = ((1280, 960),), (4,), 5, 2
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    ctx = capi.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    tris = capi.make_triangles(verts, layers=layers)
    nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts))
    ctx.upload_scene(tris, nodes, prim_idx)
    ok = True
    for w, h in sizes:
        n = w * h
        cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
        d_prim = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        ctx.generate_grid(cam, w, h, 0, h, d_prim)   # the primary rays the grid cast traces, for (a) and (b)
        rays = d_prim.cpu().numpy().view(T.RAY32)
        d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        for nl in counts:
            ls = lights(nl)
            m = n * nl
            d_rays_b = torch.from_numpy(host_rays(rays, d_hits.cpu().numpy().view(T.HIT32), ls).view(np.uint8)).cuda()
            d_occ_b = torch.empty(m, dtype=torch.uint8, device="cuda")
            d_mask_c = torch.empty(m, dtype=torch.uint8, device="cuda")
            out = {}

            def run_a():
                hits = d_hits.cpu().numpy().view(T.HIT32)  # download (on the stream, then the host waits)
                srays = host_rays(rays, hits, ls)
                occ = ctx.cast(srays, mode=capi.MODE_ANY_HIT, flags=capi.FLAG_BOOL_OUT)
                out["a"] = (1 - occ).astype(np.uint8)

            def run_b():
                ctx.cast(d_rays_b, d_occ_b, count=m, mode=capi.MODE_ANY_HIT,
                         flags=capi.FLAG_BOOL_OUT | capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE)
                out["b"] = 1 - d_occ_b

            def run_c():
                ctx.cast_grid_shadows(cam, w, h, d_hits, ls, d_mask_c)
                out["c"] = d_mask_c
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
            same = np.array_equal(out["a"], out["b"].cpu().numpy()) and np.array_equal(out["a"], out["c"].cpu().numpy())
            ok &= same
            med = {k: float(np.median(v)) for k, v in times.items()}
            for k, label in (("a", "host round trip"), ("b", "device rays + mrt_cast"), ("c", "mrt_cast_grid_shadows")):
                v = times[k]
                print(f"{w}x{h} lights={nl} pairs={m} ({k}) {label:24s} {med[k]:8.3f} ms  [{min(v):.3f} .. {max(v):.3f}]"
                      + (f"  {out['c_kernel']}" if k == "c" else ""), flush=True)
            print(f"{w}x{h} lights={nl} outputs byte-equal: {same}; lit fraction {float(out['a'].mean()):.3f}; "
                  f"(c) faster than (b): {med['c'] < med['b']} ({med['b'] / med['c']:.2f}x), than (a): {med['a'] / med['c']:.1f}x", flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
