"""Direct light of a renderer's frame on synth.room(), flat and as a two-level scene: from the primary grid's resident hit records, the
rows mrt_resolve_grid_surfaces wrote and the mask mrt_cast_grid_shadows wrote, the lit RGBA frame (with the environment: sky, ambient,
emission), produced and timed with device events on the context's stream:
  (a) the host round trip: download the records, the rows and the mask, light in numpy (messyerraytracer_amd/lighting.py, the 4 lights of
      (c)), upload the colours;
  (b) mrt_light_grid_surfaces with 1 directional light;
  (c) with 4 lights (directional, point, spot, point);
  (d) with 16 lights; (d0) the same 16 with every attenuation exponent 0, where pow01 returns at its first select: (d) - (d0) is what
      the fp64 part costs;
  (e) a device-to-device copy of as many bytes as (b) reads plus writes, the yardstick of a streaming kernel: per record 32 (record) +
      64 (row) + 1 (mask byte) read, 16 written -- 113 bytes, counted as 56.5 copied.
The variants alternate within every repeat; (a) runs in the first --host-repeats timed repeats only.  Prints one line per (scene, size,
variant): median ms and the spread (min .. max), achieved GB/s for (b) and the copy, and the share of (pixel, light) pairs that reach
pow01 (a point or spot light within range of a hit); (c)'s colours are checked byte-equal to (a)'s.
    python tools/bench_light_frame.py [--repeats 20] [--warmup 5] [--host-repeats 2] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import lighting as Lg  # noqa: E402
from bench_surface_frame import CAM, shade_data  # noqa: E402

F = np.float32
BYTES_B = 32 + 64 + 1 + 16


def light_list():
    """sixteen seeded lights in the room (x, z in [-5, 5], y in [0, 6]); the first four are (c)'s"""
    rng = np.random.default_rng(416)
    ls = np.zeros(16, T.SHADE_LIGHT)
    ls["cast_shadows"], ls["attenuation"], ls["spot_angle_attenuation"] = 1, 1, 1
    ls["color"] = rng.uniform(0.2, 3.0, size=(16, 3))
    ls["type"] = [0, 1, 2, 1] + list(rng.integers(0, 3, 12))
    ls["position"] = rng.uniform((-4, 1.5, -4), (4, 5.5, 4), size=(16, 3))
    axis = ls["position"] - rng.uniform((-3, 0, -3), (3, 1, 3), size=(16, 3))       # from a point near the floor towards the light
    ls["direction"] = axis / np.linalg.norm(axis, axis=1)[:, None]
    ls["direction"][0] = (0.3, 1.0, 0.2)
    ls["range"] = rng.uniform(4.0, 14.0, 16)
    ls["attenuation"][4:] = rng.choice([1, 2, 0.5, 3.7], 12)
    ls["attenuation"][3] = 2
    ls["spot_angle"] = rng.uniform(0.4, 1.2, 16)
    ls["spot_angle_attenuation"][4:] = rng.choice([1, 2, 0.5], 12)
    ls["spot_angle_attenuation"][2] = 0.5
    return ls


def pow_share(hits, rays, lights):
    """share of (pixel, light) pairs for which the kernel calls pow01: a point or spot light, a hit, 1e-6 <= dist <= range"""
    hit = hits["prim_id"] != -1
    p = rays["origin"][hit] + rays["direction"][hit] * hits["t"][hit, None]
    reached = 0
    for L in lights:
        if L["type"] != T.LIGHT_DIRECTIONAL:
            dist = np.linalg.norm(L["position"][None, :] - p, axis=1)
            reached += int(((dist >= 1e-6) & (dist <= L["range"])).sum())
    return reached / (hits.shape[0] * lights.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes, kinds = ((1280, 960), (1920, 1080)), ("flat", "two-level")
    if a.quick:
        sizes, kinds, a.repeats, a.warmup, a.host_repeats = ((1280, 960),), ("flat",), 5, 2, 1
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    shade = shade_data(verts)
    lights = light_list()
    plain = lights.copy()
    plain["attenuation"], plain["spot_angle_attenuation"] = 0, 0
    env = np.zeros(1, T.ENVIRONMENT)
    env["sky_zenith"], env["sky_horizon"], env["sky_ground"] = (0.15, 0.25, 0.55), (0.6, 0.7, 0.85), (0.15, 0.12, 0.1)
    env["ambient"], env["ambient_energy"] = 1.0, 0.15
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
            ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows)
            d_mask = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
            ctx.cast_grid_shadows(cam, w, h, d_hits, capi.shadow_lights(lights), d_mask)
            d_rgba_a = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
            d_rgba = {k: torch.empty(n * 16, dtype=torch.uint8, device="cuda") for k in ("b", "c", "d", "d0")}
            copy_bytes = n * BYTES_B // 2
            d_src = torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")
            d_dst = torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")

            def run_a():
                hits = d_hits.cpu().numpy().view(T.HIT32)  # downloads (on the stream, then the host waits)
                rows = d_rows.cpu().numpy().view(T.SURFACE64)
                mask = d_mask[:4 * n].cpu().numpy().reshape(4, n)
                p = rays["origin"] + rays["direction"] * hits["t"][:, None]
                rgba, _ = Lg.shade_linear(rows, hits["prim_id"] != -1, p, rays["direction"], lights[:4], mask, env[0])
                d_rgba_a.copy_(torch.from_numpy(np.ascontiguousarray(rgba).view(np.uint8).reshape(-1)))

            def lit(key, ls):
                def run():
                    ctx.light_grid_surfaces(cam, w, h, d_hits, d_rows, ls, d_rgba[key], d_mask, env[0])
                return run

            def run_copy():
                d_dst.copy_(d_src)

            variants = (("a", run_a), ("b", lit("b", lights[:1])), ("c", lit("c", lights[:4])), ("d", lit("d", lights)),
                        ("d0", lit("d0", plain)), ("e", run_copy))
            times = {k: [] for k, _ in variants}
            for rep in range(a.warmup + a.repeats):
                for v, fn in variants:
                    if v == "a" and not (rep == 0 or a.warmup <= rep < a.warmup + a.host_repeats):
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rep >= a.warmup:
                        times[v].append(e0.elapsed_time(e1))
            same = bool(torch.equal(d_rgba_a, d_rgba["c"]))
            ok &= same
            med = {k: float(np.median(v)) for k, v in times.items()}
            hits = d_hits.cpu().numpy().view(T.HIT32)
            labels = {"a": "host round trip, 4 lights", "b": "light, 1 directional", "c": "light, 4 lights", "d": "light, 16 lights",
                      "d0": "light, 16, exponents 0", "e": "device copy, (b)'s bytes"}
            for k, _ in variants:
                v = times[k]
                gbs = f"  {n * BYTES_B / med[k] / 1e6:7.0f} GB/s" if k in ("b", "e") else ""
                print(f"{kind} {w}x{h} light records={n} ({k}) {labels[k]:27s} {med[k]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}{gbs}",
                      flush=True)
            shares = [pow_share(hits, rays, ls) for ls in (lights[:1], lights[:4], lights)]
            print(f"{kind} {w}x{h} light (c) byte-equal to (a): {same}; hits {float((hits['prim_id'] != -1).mean()):.3f}; pairs reaching pow01: "
                  f"(b) {shares[0]:.3f} (c) {shares[1]:.3f} (d) {shares[2]:.3f}; (b) / (e): {med['b'] / med['e']:.2f}x; (d) / (b): "
                  f"{med['d'] / med['b']:.1f}x; (d) - (d0): {med['d'] - med['d0']:.3f} ms; (a) / (c): {med['a'] / med['c']:.0f}x", flush=True)
            del d_rows, d_mask, d_rgba, d_rgba_a, d_src, d_dst
        ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
