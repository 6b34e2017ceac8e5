"""Emitter sampling of one bounce on synth.room() at 1920x1080 (flat scene), from the primary grid's resident hit records and the rows
mrt_resolve_grid_surfaces wrote, with 2, 1024 and 2^17 emitters on the ceiling, timed with device events on the context's stream:
  the table:   mrt_build_emitters from a device array (a blocking call: wall clock);
  emitters:    mrt_cast_grid_emitter_shadows (one ray per record, to a point of the emitter it samples) + mrt_light_grid_emitter_surfaces;
  one light:   mrt_cast_grid_selected_shadows + mrt_light_grid_selected_surfaces with one point light under the ceiling, beside them.
Each call alone and each pair as one timed interval; the variants alternate within every repeat.  Prints one line per (emitter count,
variant): median ms and the spread (min .. max).
With --error: the loop of INTEGRATION 4 at 320x180, 3 bounces, the ceiling patch of tests/test_emitters_cpu.py as the only light, with and
without emitter sampling: the RMS error of the mean of F = 1, 16, 256 frames against the mean of --long frames of the sampling loop
(relative to the reference image's mean), and the two loops' time per frame.
    python tools/bench_emitter_nee.py [--repeats 20] [--warmup 5] [--quick] [--error] [--long 2048]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import path as P  # noqa: E402

CAM = ((0.0, 3.0, 4.6), (0.0, -0.35, -1.0), 70.0)
CEILING0, CELLS = 1682, 29   # synth.room(): the ceiling's first triangle, cells per side


def materials():
    m = np.zeros(2, T.MATERIAL)
    m["albedo"], m["roughness"], m["specular"] = 0.7, 0.6, 0.5
    m["emission"][1], m["emission_energy"][1] = (1.0, 0.9, 0.7), 8.0
    return m


def ceiling_ids(n_flat, cells):
    """material 1 on the first `cells` cells of a square block in the middle of the ceiling"""
    ids = np.zeros(n_flat, np.uint32)
    side = int(np.ceil(np.sqrt(cells)))
    lo = (CELLS - side) // 2
    k = 0
    for i in range(lo, lo + side):
        for j in range(lo, lo + side):
            if k < cells:
                c = CEILING0 + 2 * (i * CELLS + j)
                ids[c:c + 2] = 1
                k += 1
    return ids


def fine_ceiling(n_tris, emissive_id, size=6.0, height=6.0):
    """n_tris small triangles tiling a square of the ceiling, all carrying the id of one emissive triangle"""
    side = int(np.sqrt(n_tris // 2))
    k = np.arange(side + 1, dtype=np.float32) / np.float32(side) * np.float32(size) - np.float32(size / 2)
    x, z = np.meshgrid(k, k, indexing="ij")
    y = np.full_like(x, height)
    g = np.stack([x, y, z], axis=-1)
    p00, p10, p11, p01 = g[:-1, :-1], g[1:, :-1], g[1:, 1:], g[:-1, 1:]
    v = np.stack([np.stack([p00, p10, p11], axis=2), np.stack([p00, p11, p01], axis=2)], axis=2).reshape(-1, 3, 3)
    return capi.make_triangles(v.astype(np.float32), ids=np.full(v.shape[0], emissive_id, np.uint32))


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timings(a, ctx, stream, verts, layers, tris):
    w, h = (640, 360) if a.quick else (1920, 1080)
    n = w * h
    n_flat = verts.shape[0]
    cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
    d_hits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    d_rows = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    d_shits = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    d_mask, d_light = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    d_em = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    d_rgba = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    lamp = np.zeros(1, T.SHADE_LIGHT)
    lamp["type"], lamp["position"], lamp["color"], lamp["range"], lamp["attenuation"], lamp["cast_shadows"] = T.LIGHT_POINT, (0, 5.5, 0), (3, 3, 3), 30, 1, 1
    sh = capi.shadow_lights(lamp)
    print(f"flat synth.room() {w}x{h}: {n} records", flush=True)
    for n_emit in (2, 1024, 1 << 17):
        ids = ceiling_ids(n_flat, 1 if n_emit == 2 else 512)
        ctx.upload_shade_data(n_flat, materials(), ids)
        src = tris if n_emit <= 1024 else fine_ceiling(n_emit, int(np.flatnonzero(ids)[0]))
        d_tris = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(-1)).cuda()
        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows, None, d_shits)
        build = []
        for rep in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ctx.build_emitters(d_tris, src.shape[0], on_device=True)
            if rep >= a.warmup:
                build.append((time.perf_counter() - t0) * 1e3)
        assert got[0] == n_emit, got
        draw = T.path_emitter_draw(0)

        def em_cast():
            ctx.cast_grid_emitter_shadows(cam, w, h, d_shits, d_mask, d_em, 0, draw, flags=capi.FLAG_ASYNC)

        def em_light():
            ctx.light_grid_emitter_surfaces(cam, w, h, d_shits, d_rows, d_em, d_rgba, d_mask, 0, draw, flags=capi.FLAG_ASYNC)

        def sel_cast():
            ctx.cast_grid_selected_shadows(cam, w, h, d_shits, sh, d_mask, d_light, 0, T.path_select_draw(0), flags=capi.FLAG_ASYNC)

        def sel_light():
            ctx.light_grid_selected_surfaces(cam, w, h, d_shits, d_rows, lamp, d_light, d_rgba, d_mask, None, flags=capi.FLAG_ASYNC)

        variants = (("emitters: cast", em_cast), ("emitters: light", em_light), ("emitters: pair", lambda: (em_cast(), em_light())),
                    ("one light: cast", sel_cast), ("one light: light", sel_light), ("one light: pair", lambda: (sel_cast(), sel_light())))
        times = {k: [] for k, _ in variants}
        for rep in range(a.warmup + a.repeats):
            for k, fn in variants:
                ms = timed(stream, fn)
                if rep >= a.warmup:
                    times[k].append(ms)
        em_cast()                                                      # (the last timed call wrote the one light's bytes)
        torch.cuda.synchronize()
        em = d_em.cpu().numpy().view(np.uint32)
        lit = float(d_mask.cpu().numpy().mean())
        print(f"emitters={n_emit:6d} table build  {np.median(build):8.3f} ms  [{min(build):.3f} .. {max(build):.3f}] n={len(build)}  ({src.shape[0]} triangles, wall clock)", flush=True)
        for k, _ in variants:
            v = times[k]
            print(f"emitters={n_emit:6d} {k:17s} {np.median(v):8.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}", flush=True)
        print(f"emitters={n_emit:6d} records with an emitter {float((em != T.EMITTER_NONE).mean()):.4f}, distinct emitters {len(np.unique(em)) - 1}, "
              f"mask bytes set by the emitter cast {lit:.3f}", flush=True)


def frame(ctx, cam, w, h, bufs, env, frame_no, bounces, sample):
    """One frame of the loop, every call ASYNC; returns nothing: the state is bufs['state']."""
    A = capi.FLAG_ASYNC
    n = w * h
    b_ = bufs
    ctx.path_init(b_["state"], n, flags=A)
    ctx.cast_grid(cam, w, h, hits=b_["hits"], flags=capi.FLAG_HITS_ON_DEVICE | A)
    for b in range(bounces + 1):
        cur_rays, cur_hits = (None, b_["hits"]) if b == 0 else b_["pairs"][b & 1]
        nxt_rays, nxt_hits = b_["pairs"][(b + 1) & 1]
        draw = T.path_emitter_draw(b)
        kw = dict(frame=frame_no, bounce=b, max_bounces=bounces, d_out_lobe=b_["lobe"], flags=A)
        nee = sample and b < bounces
        if not nee:
            b_["direct"].zero_()
        if b == 0:
            ctx.resolve_grid_surfaces(cam, w, h, cur_hits, b_["rows"], b_["surf"], b_["shits"], flags=A)
            if nee:
                ctx.cast_grid_emitter_shadows(cam, w, h, b_["shits"], b_["mask"], b_["em"], frame_no, draw, flags=A)
                ctx.light_grid_emitter_surfaces(cam, w, h, b_["shits"], b_["rows"], b_["em"], b_["direct"], b_["mask"], frame_no, draw, flags=A)
            if sample:
                ctx.path_grid_step_emitters(cam, w, h, b_["shits"], b_["rows"], b_["direct"], b_["state"], env, b_["select"], None, **kw)
            else:
                ctx.path_grid_step(cam, w, h, b_["shits"], b_["rows"], b_["direct"], b_["state"], env, b_["select"], **kw)
        else:
            ctx.resolve_surfaces(cur_rays, cur_hits, n, b_["rows"], b_["surf"], b_["shits"], flags=A)
            if nee:
                ctx.cast_emitter_shadows(cur_rays, b_["shits"], n, b_["mask"], b_["em"], frame_no, draw, d_select=b_["select"], flags=A)
                ctx.light_emitter_surfaces(cur_rays, b_["shits"], b_["rows"], n, b_["em"], b_["direct"], b_["mask"], frame_no, draw, flags=A)
            if sample:
                ctx.path_step_emitters(cur_rays, b_["shits"], b_["rows"], n, b_["direct"], b_["state"], env, b_["select"], b_["lobe"], **kw)
            else:
                ctx.path_step(cur_rays, b_["shits"], b_["rows"], n, b_["direct"], b_["state"], env, b_["select"], **kw)
        if b < bounces:
            bk = dict(frame=frame_no, first_draw=P.first_draw(b), t_max=1e30, d_select=b_["select"], d_surface=b_["surf"], d_out_rays=nxt_rays, flags=A)
            if b == 0:
                ctx.cast_grid_bounce(cam, w, h, b_["shits"], nxt_hits, **bk)
            else:
                ctx.cast_bounce(cur_rays, b_["shits"], n, nxt_hits, **bk)


def errors(a, ctx, stream, verts, tris):
    w, h, bounces = 320, 180, 3
    n = w * h
    n_flat = verts.shape[0]
    cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
    ids = np.zeros(n_flat, np.uint32)
    for i in range(10, 19):
        for j in range(10, 19):
            c = CEILING0 + 2 * (i * CELLS + j)
            ids[c:c + 2] = 1
    ctx.upload_shade_data(n_flat, materials(), ids)
    print(f"error of accumulated frames, {w}x{h}, {bounces} bounces, {ctx.build_emitters(tris)[0]} emitters (the 9 x 9 cell ceiling patch), no analytic light", flush=True)
    u8 = lambda k: torch.empty(k, dtype=torch.uint8, device="cuda")
    bufs = dict(hits=u8(n * 32), rows=u8(n * 64), surf=u8(n * 8), shits=u8(n * 32), mask=u8(n), em=u8(n * 4), select=u8(n), lobe=u8(n),
                direct=torch.zeros(n * 4, dtype=torch.float32, device="cuda"), state=torch.zeros(n * 8, dtype=torch.float32, device="cuda"),
                pairs=[(u8(n * 32), u8(n * 32)), (u8(n * 32), u8(n * 32))])
    env = np.zeros(1, T.ENVIRONMENT)[0]

    def mean_of(frames, sample):
        acc = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        t0 = time.perf_counter()
        for f in frames:
            frame(ctx, cam, w, h, bufs, env, f, bounces, sample)
            acc += bufs["state"].view(n, 8)[:, 4:7].double()          # (same stream: ordered behind the frame)
        torch.cuda.synchronize()
        return (acc / len(frames)).cpu().numpy(), (time.perf_counter() - t0) * 1e3 / len(frames)

    ref, ms = mean_of(range(100000, 100000 + a.long), True)
    scale = ref.mean()
    print(f"reference: {a.long} frames of the sampling loop, {ms:.3f} ms per frame, mean radiance {scale:.4f}", flush=True)
    for F_ in (1, 16, 256):
        row = []
        for sample in (False, True):
            runs = [mean_of(range(s * 1000, s * 1000 + F_), sample) for s in range(4 if F_ < 256 else 2)]
            rms = [float(np.sqrt(((m - ref) ** 2).mean())) / scale for m, _ in runs]
            row.append((np.mean(rms), np.mean([t for _, t in runs])))
        print(f"F={F_:4d}  relative RMS error: without sampling {row[0][0]:.4f} ({row[0][1]:.3f} ms/frame), with {row[1][0]:.4f} ({row[1][1]:.3f} ms/frame); "
              f"ratio {row[0][0] / row[1][0]:.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--long", type=int, default=2048)
    a = ap.parse_args()
    if a.quick:
        a.repeats, a.warmup, a.long = 5, 2, 64
    local, inst = synth.room()
    verts = synth.flatten_instances(local, inst)
    layers = np.repeat(inst["layers"], inst["n_tris"]).astype(np.uint32)
    stream = torch.cuda.Stream()   # (a stream of its own: the default stream's handle is 0, which means the context's own stream)
    torch.cuda.set_stream(stream)
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    tris = capi.make_triangles(verts, layers=layers)
    nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(verts))
    ctx.upload_scene(tris, nodes, prim_idx)
    timings(a, ctx, stream, verts, layers, tris)
    if a.error:
        errors(a, ctx, stream, verts, tris)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
