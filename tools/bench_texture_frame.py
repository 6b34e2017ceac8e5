"""The textured surface resolve of a frame on synth.room() (flat): from the primary grid's resident hit records and resident shade data
(seeded vertex normals, UVs over 0 .. 1, 7 materials, ids i % 9, tangents for every triangle), mrt_resolve_grid_surfaces with all
three outputs, timed with device events on one stream:
  (a) nothing resident: resolve_surfaces_kernel, the yardstick;
  (b) a texture set resident whose bindings carry albedo textures only (7 RGBA8 images, one per material);
  (c) albedo textures and normal maps (14 RGBA8 images);
  (d) a device-to-device copy of as many bytes as (c) reads plus writes: per record (a)'s 248, one 16-byte binding, one 48-byte tangent
      row and per sampled texture one 16-byte descriptor and four 4-byte texels -- 376 bytes, counted as 188 copied;
(b) to (d) with images of 256 x 256 (256 KiB each: the set fits the caches) and of 4096 x 4096 (64 MiB each: one image exceeds L2, the
set exceeds the Infinity Cache).  Every variant has a context of its own (the set is the context's), all on one stream, sharing the
records; the variants alternate within every repeat.  Prints one line per (size, variant): median ms and the spread (min .. max), and
the ratios (b)/(a), (c)/(a), (c)/(d); (c)'s rows at 256 x 256 are checked against messyerraytracer_amd/texture.py once per size.
    python tools/bench_texture_frame.py [--repeats 20] [--warmup 5] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import texture as X  # noqa: E402
from bench_surface_frame import CAM, shade_data  # noqa: E402

F = np.float32
BYTES_PLAIN = 32 + 64 + 48 + 64 + 8 + 32
BYTES_TEXTURED = BYTES_PLAIN + 16 + 48 + 2 * (16 + 4 * 4)
N_MATERIALS = 7


def texture_set(dim, normals, n_tris):
    rng = np.random.default_rng(418 + dim)
    n_tex = N_MATERIALS * (2 if normals else 1)
    images = [rng.integers(0, 256, size=(dim, dim, 4), dtype=np.uint8) for _ in range(n_tex)]
    b = X.bindings(list(range(N_MATERIALS)), [N_MATERIALS + m if normals else None for m in range(N_MATERIALS)], np.ones(N_MATERIALS, F))
    t = np.random.default_rng(419).normal(size=(n_tris, 3, 3))
    t /= np.linalg.norm(t, axis=2)[:, :, None]
    tan = np.concatenate([t.reshape(n_tris, 9), np.ones((n_tris, 3))], axis=1).astype(F)
    return X.TextureSet(images, b, tan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes, dims = ((1280, 960), (1920, 1080)), (256, 4096)
    if a.quick:
        sizes, dims, a.repeats, a.warmup = ((1280, 960),), (256,), 5, 2
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    shade = shade_data(verts)
    stream = torch.cuda.current_stream()
    ctxs, sets = {}, {}
    names = ["a"] + [f"{v}{d}" for d in dims for v in "bc"]
    for name in names:
        ctx = capi.Context(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
        if name != "a":
            sets[name] = texture_set(int(name[1:]), name[0] == "c", shade.n_tris)
            ctx.upload_textures(sets[name].textures, sets[name].bindings, sets[name].tangents12)
            if name != "c256":
                sets[name] = None  # (only c256 is checked: drop the host copies)
        ctxs[name] = ctx
    caster = ctxs["a"]
    tris = capi.make_triangles(verts, layers=layers)
    nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts))
    caster.upload_scene(tris, nodes, prim_idx)
    ok = True
    for w, h in sizes:
        n = w * h
        cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
        d_prim = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        caster.generate_grid(cam, w, h, 0, h, d_prim)
        rays = d_prim.cpu().numpy().view(T.RAY32)
        d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        caster.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        hits = d_hits.cpu().numpy().view(T.HIT32)
        out = {k: (torch.empty(n * 64, dtype=torch.uint8, device="cuda"), torch.empty(n * 8, dtype=torch.uint8, device="cuda"),
                   torch.empty(n * 32, dtype=torch.uint8, device="cuda")) for k in names}
        copy_bytes = n * BYTES_TEXTURED // 2
        d_src = torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")
        d_dst = torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")

        def resolve(name):
            return lambda: ctxs[name].resolve_grid_surfaces(cam, w, h, d_hits, *out[name])

        variants = [(k, resolve(k)) for k in names] + [("d", lambda: d_dst.copy_(d_src))]
        times = {k: [] for k, _ in variants}
        for rep in range(a.warmup + a.repeats):
            for v, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    times[v].append(e0.elapsed_time(e1))
        want, _, _ = X.resolve_textured(rays["direction"], hits["normal"], hits["prim_id"] != -1, hits["prim_id"].view(np.uint32),
                                        hits["bary_u"], hits["bary_v"], shade, sets["c256"])
        same = bool(np.array_equal(out["c256"][0].cpu().numpy().view(np.uint32), want.view(np.uint32)))
        ok &= same
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k, _ in variants:
            v = times[k]
            label = {"a": "(a) nothing resident", "b": "(b) albedo textures", "c": "(c) albedo and normal maps", "d": "(d) device copy, (c)'s bytes"}[k[0]]
            dim = f" {k[1:]}^2" if k[1:] else ""
            print(f"flat {w}x{h} records={n} {label + dim:36s} {med[k]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}", flush=True)
        ratios = "; ".join(f"{d}^2: (b)/(a) {med[f'b{d}'] / med['a']:.2f}x, (c)/(a) {med[f'c{d}'] / med['a']:.2f}x, (c)/(d) {med[f'c{d}'] / med['d']:.2f}x" for d in dims)
        print(f"flat {w}x{h} (c) 256^2 rows equal texture.py: {same}; hits {float((hits['prim_id'] != -1).mean()):.3f}; {ratios}", flush=True)
        del out, d_src, d_dst
    for ctx in ctxs.values():
        ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
