"""The channel passes of a RayRenderer frame on synth.room() (flat): from the primary grid's resident hit records, resident shade data
(seeded vertex normals, UVs, 7 materials, ids i % 9) and a resident texture set (bindings for 5 of the 7 materials, tangents for every
triangle), the renderer's channels produced several ways and timed with device events on the context's stream:
  (a) the host round trip: download the records, shade all ten channels in numpy (messyerraytracer_amd/channels.py) and convert them
      with to_rgba8, upload the ten byte planes;
  (b_depth) mrt_shade_grid_channels with DEPTH alone, float plane: per record 32 bytes read (the record; the ray is made again) and 16
      written -- 48;
  (b_normal) the same with NORMAL alone, float plane: 32 + 64 (shade row of a hit in range) read, 16 written -- 112, not counting the
      binding, the tangents and the texels of the records a normal map applies to;
  (c) all ten channels, float and byte planes: 32 + 64 + 16 (the material's first word) read, 10 x (16 + 4) written -- 312, with the
      same omission;
  (finish) mrt_finish_color, ACES, float and byte output: 16 read, 20 written -- 36;
  (copy_*) a device-to-device copy of as many bytes as each kernel reads plus writes (half of them copied), the yardstick of a
      streaming kernel, in the same run.
The variants alternate within every repeat; (a) runs in the first --host-repeats timed repeats only.  Prints one line per (size,
variant): median ms and the spread (min .. max), achieved GB/s for the kernels and the copies; (c)'s byte planes are checked byte-equal
to (a)'s.
    python tools/bench_channel_frame.py [--repeats 20] [--warmup 5] [--host-repeats 3] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import channels as Ch  # noqa: E402
from messyerraytracer_amd import surface as S  # noqa: E402
from messyerraytracer_amd import texture as X  # noqa: E402

F = np.float32
CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
INV_POS = F(1) / F(0.75)
BYTES = {"b_depth": 32 + 16, "b_normal": 32 + 64 + 16, "c": 32 + 64 + 16 + 10 * 20, "finish": 16 + 20}


def shade_data(verts):
    v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3, 3)
    n = v.shape[0]
    rng = np.random.default_rng(421)
    face = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    face /= np.maximum(np.linalg.norm(face, axis=1), 1e-30)[:, None]
    vn = face[:, None, :] + 0.35 * rng.normal(size=(n, 3, 3))
    vn /= np.linalg.norm(vn, axis=2)[:, :, None]
    m = np.zeros(7, T.MATERIAL)
    m["albedo"] = rng.uniform(0.05, 0.95, size=(7, 3))
    m["roughness"], m["specular"] = 0.5, 0.5
    shade = S.ShadeData(n, m, (np.arange(n) % 9).astype(np.uint32), vn.astype(F), rng.uniform(-3, 3, size=(n, 3, 2)).astype(F))
    images = [rng.integers(0, 256, size=(64, 64, 4), dtype=np.uint8), rng.uniform(0, 1, size=(16, 32, 4)).astype(F),
              rng.integers(0, 256, size=(8, 8, 4), dtype=np.uint8)]
    t = rng.normal(size=(n, 3, 3))
    t /= np.linalg.norm(t, axis=2)[:, :, None]
    tan = np.concatenate([t.reshape(n, 9), np.ones((n, 3))], axis=1).astype(F)
    tex = X.TextureSet(images, X.bindings([0, 1, None, 2, None], [2, None, 0, 1, None], [1.0, 2.0, 4.0, 0.5, 1.0]), tan)
    return shade, tex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes = ((1280, 960), (1920, 1080))
    if a.quick:
        sizes, a.repeats, a.warmup, a.host_repeats = ((1280, 960),), 5, 2, 1
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    shade, tex = shade_data(verts)
    stream = torch.cuda.current_stream()
    ok = True
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    tris = capi.make_triangles(verts, layers=layers)
    nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts))
    ctx.upload_scene(tris, nodes, prim_idx)
    ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
    ctx.upload_textures(tex.textures, tex.bindings, tex.tangents12)
    for w, h in sizes:
        n = w * h
        cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
        d_prim = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        ctx.generate_grid(cam, w, h, 0, h, d_prim)
        rays = d_prim.cpu().numpy().view(T.RAY32)
        d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        hits0 = d_hits.cpu().numpy().view(T.HIT32)
        inv_d = F(1) / F(np.median(hits0["t"][hits0["prim_id"] != -1]))
        rgba = {c: torch.empty(n * 16, dtype=torch.uint8, device="cuda") for c in Ch.ALL}
        rgba8 = {c: torch.empty(n * 4, dtype=torch.uint8, device="cuda") for c in Ch.ALL}
        host8 = {c: torch.empty(n * 4, dtype=torch.uint8, device="cuda") for c in Ch.ALL}
        d_fin = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        d_fin8 = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
        copies = {k: (torch.empty(n * b // 2, dtype=torch.uint8, device="cuda"), torch.empty(n * b // 2, dtype=torch.uint8, device="cuda"))
                  for k, b in BYTES.items()}

        def run_a():
            hits = d_hits.cpu().numpy().view(T.HIT32)  # download (on the stream, then the host waits)
            planes = Ch.shade_channels(rays["direction"], Ch.hit_position(rays["origin"], rays["direction"], hits["t"]), hits["normal"],
                                       hits["prim_id"] != -1, hits["t"], hits["prim_id"].view(np.uint32), hits["bary_u"], hits["bary_v"],
                                       inv_d, INV_POS, shade, tex)
            for c in Ch.ALL:
                host8[c].copy_(torch.from_numpy(Ch.to_rgba8(planes[c]).reshape(-1)))

        def run_b_depth():
            ctx.shade_grid_channels(cam, w, h, d_hits, inv_d, INV_POS, {Ch.DEPTH: rgba[Ch.DEPTH]})

        def run_b_normal():
            ctx.shade_grid_channels(cam, w, h, d_hits, inv_d, INV_POS, {Ch.NORMAL: rgba[Ch.NORMAL]})

        def run_c():
            ctx.shade_grid_channels(cam, w, h, d_hits, inv_d, INV_POS, rgba, rgba8)

        def run_finish():
            ctx.finish_color(rgba[Ch.ALBEDO], n, d_fin, d_fin8, tonemap_mode=3)

        def copy(k):
            return lambda: copies[k][1].copy_(copies[k][0])

        variants = [("a", run_a), ("b_depth", run_b_depth), ("copy_b_depth", copy("b_depth")), ("b_normal", run_b_normal),
                    ("copy_b_normal", copy("b_normal")), ("c", run_c), ("copy_c", copy("c")), ("finish", run_finish), ("copy_finish", copy("finish"))]
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
        same = all(bool(torch.equal(host8[c], rgba8[c])) for c in Ch.ALL)
        ok &= same
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k, _ in variants:
            v = times[k]
            b = BYTES.get(k.replace("copy_", ""))
            gbs = f"  {n * b / med[k] / 1e6:7.0f} GB/s" if b else ""
            print(f"flat {w}x{h} channels records={n} ({k}) {med[k]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}{gbs}", flush=True)
        print(f"flat {w}x{h} channels byte planes byte-equal to the host's: {same}; hits {float((hits0['prim_id'] != -1).mean()):.3f}; kernel / copy: "
              + "; ".join(f"{k} {med[k] / med['copy_' + k]:.2f}x" for k in BYTES) + f"; (a) / (c): {med['a'] / med['c']:.0f}x", flush=True)
        del rgba, rgba8, host8, d_fin, d_fin8, copies
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
