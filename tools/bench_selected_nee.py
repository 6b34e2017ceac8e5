"""Next-event estimation of one bounce on synth.room() at 1920x1080 (flat scene), from the primary grid's resident hit records and the
rows mrt_resolve_grid_surfaces wrote, two ways, with 1, 4 and 16 lights, timed with device events on the context's stream:
  all lights:  mrt_cast_grid_shadows (n_lights rays per record) + mrt_light_grid_surfaces (the loop over the lights);
  one light:   mrt_cast_grid_selected_shadows (one ray per record, to the light it draws) + mrt_light_grid_selected_surfaces.
Each call alone and each pair as one timed interval; the six variants of a light count alternate within every repeat.  Prints one line
per (light count, variant): median ms, the spread (min .. max) and the rays traced, and per light count the ratio of the two pairs with
the two spreads beside it.  The selected lit bytes are checked against the all-lights mask's byte of the same (record, light) pair.
    python tools/bench_selected_nee.py [--repeats 20] [--warmup 5] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from bench_light_frame import light_list  # noqa: E402
from bench_surface_frame import CAM, shade_data  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    w, h = (1920, 1080)
    if a.quick:
        w, h, a.repeats, a.warmup = 640, 360, 5, 2
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    shade = shade_data(verts)
    lights = light_list()
    stream = torch.cuda.current_stream()
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    tris = capi.make_triangles(verts, layers=layers)
    nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts))
    ctx.upload_scene(tris, nodes, prim_idx)
    ctx.upload_shade_data(shade.n_tris, shade.materials, shade.material_ids, shade.normals9, shade.uvs6)
    n = w * h
    cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
    d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
    d_rows = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows)
    hit_share = float((d_hits.cpu().numpy().view(T.HIT32)["prim_id"] != -1).mean())
    d_all = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    d_mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_light = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_rgba = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    ok = True
    print(f"flat synth.room() {w}x{h}: {n} records, hits {hit_share:.3f}", flush=True)
    for n_lights in (1, 4, 16):
        ls = lights[:n_lights]
        sh = capi.shadow_lights(ls)

        def shadows_all():
            ctx.cast_grid_shadows(cam, w, h, d_hits, sh, d_all)

        def light_all():
            ctx.light_grid_surfaces(cam, w, h, d_hits, d_rows, ls, d_rgba, d_all, None)

        def shadows_one():
            ctx.cast_grid_selected_shadows(cam, w, h, d_hits, sh, d_mask, d_light, 0, T.path_select_draw(0))

        def light_one():
            ctx.light_grid_selected_surfaces(cam, w, h, d_hits, d_rows, ls, d_light, d_rgba, d_mask, None)

        def pair_all():
            shadows_all()
            light_all()

        def pair_one():
            shadows_one()
            light_one()

        variants = (("all: shadows", shadows_all), ("all: light", light_all), ("all: pair", pair_all),
                    ("one: shadows", shadows_one), ("one: light", light_one), ("one: pair", pair_one))
        times = {k: [] for k, _ in variants}
        names = {}
        for rep in range(a.warmup + a.repeats):
            for k, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
                if "shadows" in k:
                    names[k] = ctx.last_kernel_variant()
        # the selected byte is the all-lights mask's byte of the pair
        allm, mask, lb = d_all[:n * n_lights].cpu().numpy(), d_mask.cpu().numpy(), d_light.cpu().numpy()
        on = lb != T.LIGHT_NONE
        same = bool((mask[~on] == 1).all() and np.array_equal(mask[on], allm[lb[on].astype(np.int64) * n + np.flatnonzero(on)]))
        ok &= same
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k, _ in variants:
            v = times[k]
            rays = "" if "light" in k else f"  rays {n * (n_lights if k.startswith('all') else 1)}  {names.get(k, '')}"
            print(f"lights={n_lights:2d} {k:13s} {med[k]:8.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}{rays}", flush=True)
        sa, so = times["all: pair"], times["one: pair"]
        print(f"lights={n_lights:2d} all pair / one pair: {med['all: pair'] / med['one: pair']:.2f}x; spread of the all pair {max(sa) - min(sa):.3f} ms, "
              f"of the one pair {max(so) - min(so):.3f} ms; one - all: {med['one: pair'] - med['all: pair']:+.3f} ms; selected bytes equal the pairs' "
              f"bytes: {same}", flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
