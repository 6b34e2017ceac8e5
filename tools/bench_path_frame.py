"""The path tracer's per-pixel bookkeeping on synth.room(), flat and as a two-level scene, timed with device events on the context's
stream from the primary grid's resident records, rows, bounce pairs and direct light (4 lights, env = NULL):
  (a) what a host-driven loop needs for one bounce's bookkeeping: download the direct light, the rows and the lobe bytes, step in numpy
      (messyerraytracer_amd/path.py), upload the select bytes;
  (b) mrt_path_grid_step at bounce 0 from mrt_path_init's state, (b2) at bounce 2 (roulette) from the same state, (b0) bounce 0 without
      d_active_count: (b) - (b0) is what the one atomic add per wave costs;
  (c) a device-to-device copy of as many bytes as (b) moves, the yardstick of a streaming kernel: per record 32 (state) + 64 (row) + 16
      (direct) + 32 (record) read, 32 + 2 written -- 178 bytes, counted as 89 copied;
  (d) a four-bounce frame end to end -- primary cast, init, per bounce resolve -> shadows -> light -> step -> bounce cast, one 4-byte
      read-back per bounce, finish -- with the step's select bytes fed to the bounce cast, and (d1) the same frame with select all ones
      (ended paths keep tracing): (d1) - (d) is what roulette and stopped paths save in tracing.
The state is set again outside the timed region before every (b) / (b2); the variants alternate within every repeat; (a) runs in the
first --host-repeats timed repeats only.  Prints one line per (scene, size, variant): median ms and the spread (min .. max), GB/s for (b)
and the copy; (a)'s select bytes are checked byte-equal to (b)'s, and the entries left active after each bounce of (d) are printed.
    python tools/bench_path_frame.py [--repeats 20] [--warmup 5] [--host-repeats 2] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402
from messyerraytracer_amd import path as P  # noqa: E402
from bench_light_frame import light_list  # noqa: E402
from bench_surface_frame import CAM, shade_data  # noqa: E402

F = np.float32
BYTES_B = 32 + 64 + 16 + 32 + 32 + 2
FRAME, BOUNCES, FAR = 3, 4, 1e30


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
    lights = light_list()[:4]
    shadow = capi.shadow_lights(lights)
    env = np.zeros(1, T.ENVIRONMENT)
    env["sky_zenith"], env["sky_horizon"], env["sky_ground"] = (0.15, 0.25, 0.55), (0.6, 0.7, 0.85), (0.15, 0.12, 0.1)
    env["ambient"], env["ambient_energy"] = 1.0, 0.15
    stream = torch.cuda.Stream()   # a stream of its own: torch's copies and read-backs and the library's ASYNC calls queue on the same one
    A = capi.FLAG_ASYNC
    ok = True
    with torch.cuda.stream(stream):
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

                def buf(nbytes):
                    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")

                cam = capi.camera_look(CAM[0], CAM[1], w, h, CAM[2])
                d_prim = buf(n * 32)
                ctx.generate_grid(cam, w, h, 0, h, d_prim)
                rays = d_prim.cpu().numpy().view(T.RAY32)
                d_hits, d_rows, d_pairs, d_shits, d_mask, d_direct = buf(n * 32), buf(n * 64), buf(n * 8), buf(n * 32), buf(n * 4), buf(n * 16)
                d_state, d_fresh, d_select, d_lobe, d_ones, d_rgba = buf(n * 32), buf(n * 32), buf(n), buf(n), torch.ones(n, dtype=torch.uint8, device="cuda"), buf(n * 16)
                d_select_a = buf(n)
                d_counts = torch.zeros(8, dtype=torch.int32, device="cuda")
                pairs = [(buf(n * 32), buf(n * 32)), (buf(n * 32), buf(n * 32))]       # (rays, records) of the odd and the even bounces
                d_src, d_dst = buf(n * BYTES_B // 2), buf(n * BYTES_B // 2)
                pixel = np.arange(n, dtype=np.uint64)

                def primary_chain():
                    ctx.resolve_grid_surfaces(cam, w, h, d_hits, d_rows, d_pairs, d_shits, flags=A)
                    ctx.cast_grid_shadows(cam, w, h, d_hits, shadow, d_mask, flags=A)
                    ctx.light_grid_surfaces(cam, w, h, d_hits, d_rows, lights, d_direct, d_mask, None, flags=A)

                ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                primary_chain()
                ctx.path_init(d_fresh, n)
                state_host = d_fresh.cpu().numpy().view(T.PATH_STATE)

                def run_a():
                    direct = d_direct.cpu().numpy().view(F).reshape(-1, 4)            # downloads (on the stream, then the host waits)
                    rows = d_rows.cpu().numpy().view(T.SURFACE64)
                    d_lobe.cpu()                                                       # (what a host-driven loop reads to know the lobe sampled)
                    _, select, _, _ = P.path_step(state_host, rows, rows["n_dot_v"] > 0, rows["normal"], rays["direction"], direct, env[0], pixel,
                                                  FRAME, 0, BOUNCES)
                    d_select_a.copy_(torch.from_numpy(select))

                def step(bounce, count=True):
                    def run():
                        ctx.path_grid_step(cam, w, h, d_shits, d_rows, d_direct, d_state, env[0], d_select, FRAME, bounce, BOUNCES, d_lobe,
                                           d_counts[7:8] if count else None, flags=A)
                    return run

                def run_copy():
                    d_dst.copy_(d_src)

                active = {}

                def frame(key, culled):
                    def run():
                        ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE | A)
                        ctx.path_init(d_state, n, flags=A)
                        d_counts.zero_()
                        left = []
                        for b in range(BOUNCES + 1):
                            cur_rays, cur_hits = (None, d_hits) if b == 0 else pairs[b & 1]
                            nxt_rays, nxt_hits = pairs[(b + 1) & 1]
                            kw = dict(frame=FRAME, bounce=b, max_bounces=BOUNCES, d_out_lobe=d_lobe, d_active_count=d_counts[b:b + 1], flags=A)
                            if b == 0:
                                primary_chain()
                                ctx.path_grid_step(cam, w, h, d_shits, d_rows, d_direct, d_state, env[0], d_select, **kw)
                            else:
                                ctx.resolve_surfaces(cur_rays, cur_hits, n, d_rows, d_pairs, d_shits, flags=A)
                                ctx.cast_shadows(cur_rays, cur_hits, n, shadow, d_mask, flags=A)
                                ctx.light_surfaces(cur_rays, cur_hits, d_rows, n, lights, d_direct, d_mask, None, flags=A)
                                ctx.path_step(cur_rays, d_shits, d_rows, n, d_direct, d_state, env[0], d_select, **kw)
                            left.append(int(d_counts[b:b + 1].cpu()[0]))               # the loop's one read-back
                            if left[-1] == 0:
                                break
                            bk = dict(frame=FRAME, first_draw=P.first_draw(b), t_max=FAR, d_select=d_select if culled else d_ones, d_surface=d_pairs,
                                      d_out_rays=nxt_rays, flags=A)
                            if b == 0:
                                ctx.cast_grid_bounce(cam, w, h, d_shits, nxt_hits, **bk)
                            else:
                                ctx.cast_bounce(cur_rays, d_shits, n, nxt_hits, **bk)
                        ctx.path_finish(d_state, n, d_rgba, 3, flags=A)
                        active[key] = left
                    return run

                variants = (("a", run_a), ("b", step(0)), ("b2", step(2)), ("b0", step(0, False)), ("c", run_copy), ("d", frame("d", True)), ("d1", frame("d1", False)))
                times = {k: [] for k, _ in variants}
                frames = {}
                for rep in range(a.warmup + a.repeats):
                    for v, fn in variants:
                        if v == "a" and not (rep == 0 or a.warmup <= rep < a.warmup + a.host_repeats):
                            continue
                        if v in ("b", "b2", "b0"):
                            d_state.copy_(d_fresh)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        fn()
                        e1.record(stream)
                        e1.synchronize()
                        if rep >= a.warmup:
                            times[v].append(e0.elapsed_time(e1))
                        if v == "b":
                            sel_b = d_select.clone()
                        if v in ("d", "d1"):                                        # put bounce 0's rows and direct light back for (a), (b), (b2)
                            frames[v] = d_rgba.clone()
                            ctx.cast_grid(cam, w, h, hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
                            primary_chain()
                            ctx.synchronize()
                same = bool(torch.equal(d_select_a, sel_b))
                same_frame = bool(torch.equal(frames["d"], frames["d1"]))
                ok &= same and same_frame
                med = {k: float(np.median(v)) for k, v in times.items()}
                labels = {"a": "host bookkeeping, one bounce", "b": "step, bounce 0", "b2": "step, bounce 2", "b0": "step, bounce 0, no count", "c": "device copy, (b)'s bytes",
                          "d": "4-bounce frame, step's select", "d1": "4-bounce frame, select all 1"}
                for k, _ in variants:
                    v = times[k]
                    gbs = f"  {n * BYTES_B / med[k] / 1e6:7.0f} GB/s" if k in ("b", "b2", "b0", "c") else ""
                    print(f"{kind} {w}x{h} path records={n} ({k}) {labels[k]:30s} {med[k]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}] n={len(v)}{gbs}", flush=True)
                print(f"{kind} {w}x{h} path (a)'s select byte-equal to (b)'s: {same}; (d) and (d1) finish the same frame: {same_frame}; active after each "
                      f"bounce of (d): {active['d']} of {n}; (b) / (c): {med['b'] / med['c']:.2f}x; (b2) / (c): {med['b2'] / med['c']:.2f}x; (b0) / (c): {med['b0'] / med['c']:.2f}x; "
                      f"(d1) - (d): {med['d1'] - med['d']:.3f} ms ({med['d1'] / med['d']:.2f}x); (a) / (b): {med['a'] / med['b']:.0f}x", flush=True)
            ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
