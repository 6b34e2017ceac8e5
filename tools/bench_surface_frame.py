"""The surface resolve of a path tracer's frame on synth.room(), flat and as a two-level scene: from the primary grid's resident hit
records and resident shade data (seeded vertex normals, UVs, 7 materials, ids i % 9), the {metallic, roughness} pairs
mrt_cast_grid_bounce takes, produced two ways and timed with device events on the context's stream:
  (a) the host round trip: download the records, resolve in numpy (messyerraytracer_amd/surface.py), upload the pairs;
  (b) mrt_resolve_grid_surfaces with all three outputs (rows, pairs, records with the shading normal);
  (copy) a device-to-device copy of as many bytes as (b) reads plus writes, the yardstick of a streaming kernel: per record 32 (record)
      + 64 (shade row of a hit in range) + 48 (material) read, 64 + 8 + 32 written -- 248 bytes, counted as 124 copied;
and a bounce frame with and without the round trip: grid cast, then (a) or (b), then mrt_cast_grid_bounce with the pairs.
The variants alternate within every repeat; (a) runs in the first --host-repeats timed repeats only.  Prints one line per (scene, size,
variant): median ms and the spread (min .. max), achieved GB/s for (b) and the copy; (b)'s pairs are checked byte-equal to (a)'s.
    python tools/bench_surface_frame.py [--repeats 20] [--warmup 5] [--host-repeats 3] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import surface as S  # noqa: E402

F = np.float32
CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
FRAME, T_MAX = 1, F(1e30)
BYTES_PER_RECORD = 32 + 64 + 48 + 64 + 8 + 32


def shade_data(verts):
    v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3, 3)
    n = v.shape[0]
    rng = np.random.default_rng(415)
    face = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    face /= np.maximum(np.linalg.norm(face, axis=1), 1e-30)[:, None]
    vn = face[:, None, :] + 0.35 * rng.normal(size=(n, 3, 3))
    vn /= np.linalg.norm(vn, axis=2)[:, :, None]
    m = np.zeros(7, T.MATERIAL)
    m["albedo"] = rng.uniform(0.05, 0.95, size=(7, 3))
    m["metallic"] = [0.0, 0.5, 1.0, 0.25, 0.0, 1.0, 0.75]
    m["roughness"] = [0.02, 0.3, 1.0, 0.04, 0.0, 0.6, 0.039]
    m["specular"] = 0.5
    m["emission_energy"] = [0.0, 3.5, 0.0, 0.0, 12.0, 0.0, 0.0]
    m["emission"] = 1.0
    return S.ShadeData(n, m, (np.arange(n) % 9).astype(np.uint32), vn.astype(F), rng.uniform(0, 1, size=(n, 3, 2)).astype(F))


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
    shade = shade_data(verts)
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
        ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
        for w, h in sizes:
            n = w * h
            cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
            d_prim = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            ctx.generate_grid(cam, w, h, 0, h, d_prim)
            rays = d_prim.cpu().numpy().view(T.RAY32)
            d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
            d_rows = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            d_pairs_a = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
            d_pairs_b = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
            d_smooth = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            d_bounce = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            copy_bytes = n * BYTES_PER_RECORD // 2
            d_src = torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")
            d_dst = torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")

            def run_a():
                hits = d_hits.cpu().numpy().view(T.HIT32)  # download (on the stream, then the host waits)
                _, pairs, _ = S.resolve(rays["direction"], hits["normal"], hits["prim_id"] != -1, hits["prim_id"].view(np.uint32),
                                        hits["bary_u"], hits["bary_v"], shade)
                d_pairs_a.copy_(torch.from_numpy(np.ascontiguousarray(pairs).view(np.uint8).reshape(-1)))

            def run_b():
                ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows, d_pairs_b, d_smooth)

            def run_copy():
                d_dst.copy_(d_src)

            def frame(resolve, d_pairs):
                def run():
                    ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                    resolve()
                    ctx.cast_grid_bounce(cam, w, h, d_hits, d_bounce, frame=FRAME, t_max=T_MAX, d_surface=d_pairs)
                return run

            variants = (("a", run_a), ("b", run_b), ("copy", run_copy), ("frame_a", frame(run_a, d_pairs_a)), ("frame_b", frame(run_b, d_pairs_b)))
            times = {k: [] for k, _ in variants}
            for rep in range(a.warmup + a.repeats):
                for v, fn in variants:
                    if v in ("a", "frame_a") and not (rep == 0 or a.warmup <= rep < a.warmup + a.host_repeats):
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        times[v].append(e0.elapsed_time(e1))
            same = bool(torch.equal(d_pairs_a, d_pairs_b))
            ok &= same
            med = {k: float(np.median(v)) for k, v in times.items()}
            hits = d_hits.cpu().numpy().view(T.HIT32)
            labels = {"a": "host round trip", "b": "mrt_resolve_grid_surfaces", "copy": "device copy, same bytes",
                      "frame_a": "frame: grid, (a), bounce", "frame_b": "frame: grid, (b), bounce"}
            for k, _ in variants:
                v = times[k]
                gbs = f"  {n * BYTES_PER_RECORD / med[k] / 1e6:7.0f} GB/s" if k in ("b", "copy") else ""
                print(f"{kind} {w}x{h} surface records={n} ({k}) {labels[k]:27s} {med[k]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}{gbs}",
                      flush=True)
            print(f"{kind} {w}x{h} surface pairs byte-equal: {same}; hits {float((hits['prim_id'] != -1).mean()):.3f}; (b) / copy: "
                  f"{med['b'] / med['copy']:.2f}x; (a) / (b): {med['a'] / med['b']:.0f}x; frame (a) / frame (b): "
                  f"{med['frame_a'] / med['frame_b']:.0f}x", flush=True)
            del d_rows, d_pairs_a, d_pairs_b, d_smooth, d_bounce, d_src, d_dst
        ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
