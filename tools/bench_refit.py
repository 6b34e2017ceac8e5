"""What a refit costs and what it does to the trace, against the rebuilds a moving scene would otherwise pay.
Scenes: C3 (the 1 M-triangle soup, host SAH tree uploaded), C5 (64 instanced meshes, 10 M triangles, built on the device) and
synth.room() (11 076 triangles, host SAH tree).  Frames come from synth.deform.  Per scene:
  refit      mrt_refit_scene (C5: mrt_refit_instanced_scene, meshes resident) between two frames: device time (last_build_ms) and
             host wall time around the blocking call, median over --repeats after --warmup; triangles already on the device;
  rebuild    the same frame through mrt_build_scene_device (radix tree, SAH; device time and wall) and the host SAH builder +
             upload (wall; C5 once);
  identity   the config's grid (mrt_cast_grid) and 2^22 incoherent device-resident rays on a scene refit with its own triangles
             against the same scene never refit (two contexts, alternating casts, device events on one stream);
  motion     deformations of growing amplitude: trace times after a refit of the frame-0 tree against a fresh SAH build of the same
             frame (device SAH builder: the host builder's tree), records checked byte-equal.
    python tools/bench_refit.py [--configs C3,C5,room] [--repeats 20] [--warmup 3] [--json OUT]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402

ROOM_CAM = dict(grid=(1280, 960), origin=(0.0, 3.0, 4.6), forward=(0.0, -0.35, -1.0), fov=70.0)
AMPLITUDES = (0.0, 0.002, 0.01, 0.05, 0.2, 1.0)  # in scene units (C3 / C5 span [-5, 5]^3; the room is 10 x 6 x 10)


def med(v):
    return float(np.median(v)) if v else float("nan")


class Scene:
    """one config: how to load its frame 0 and how to refit / rebuild a frame"""

    def __init__(self, name):
        self.name = name
        if name == "C5":
            cfg = synth.CONFIGS["C5"]
            self.local, self.inst = synth.multi_mesh_instances(cfg["n_meshes"], cfg["tris_per_mesh"], cfg["s"], cfg["seed"])
            self.layers = None
            self.cam = cfg
            self.grid = (2048, 2048)  # (the 8192^2 grid of bench.py takes 20 ms a cast; the ratio is what is wanted here)
        else:
            if name == "room":
                self.local, self.inst = synth.room()
                self.layers = np.repeat(self.inst["layers"], self.inst["n_tris"]).astype(np.uint32)
                self.cam = ROOM_CAM
            else:
                cfg = synth.CONFIGS[name]
                self.local, self.inst, self.layers, self.cam = synth.scene_vertices(cfg), None, None, cfg
            self.grid = self.cam["grid"]

    def world(self, local):
        return local if self.inst is None else synth.flatten_instances(local, self.inst)

    def frame(self, amplitude, phase):
        return synth.deform(self.local, amplitude, phase, seed=7)

    def tris(self, local):
        return capi.make_triangles(self.world(local), None, self.layers)

    def load(self, ctx, local):
        """frame `local` as the config builds it: a host SAH tree (C3, room) or the instanced device build (C5)"""
        if self.inst is not None:
            ctx.build_instanced_scene_device(local, self.inst)
        else:
            tris = self.tris(local)
            nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(self.world(local)))
            ctx.upload_scene(tris, nodes, prim_idx)

    def device_input(self, local):
        """what a refit reads, resident: the mesh vertices (C5) or the triangles"""
        a = local if self.inst is not None else self.tris(local)
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    def refit(self, ctx, d_in):
        if self.inst is not None:
            ctx.refit_instanced_scene(d_in, self.inst, n_mesh_tris=self.local.shape[0], on_device=True)
        else:
            ctx.refit_scene(d_in, n_tris=self.local.shape[0], on_device=True)


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def trace_pair(sc, ctxs, stream, repeats, warmup):
    """grid and incoherent trace ms of every context, alternating; returns ({name: [grid ms]}, {name: [inc ms]}, records equal)"""
    w, h = sc.grid
    cam = capi.camera_look(sc.cam["origin"], sc.cam["forward"], w, h, sc.cam["fov"])
    inc = synth.incoherent_rays(1 << 22, 7)
    d_inc = torch.from_numpy(inc.view(np.uint8).reshape(-1)).cuda()
    outs = {k: (torch.empty(w * h * 32, dtype=torch.uint8, device="cuda"), torch.empty(inc.shape[0] * 32, dtype=torch.uint8, device="cuda")) for k in ctxs}
    tg, ti = {k: [] for k in ctxs}, {k: [] for k in ctxs}
    for rep in range(warmup + repeats):
        for k, c in ctxs.items():
            g = timed(stream, lambda: c.cast_grid(cam, w, h, hits=outs[k][0], flags=capi.FLAG_HITS_ON_DEVICE))
            i = timed(stream, lambda: c.cast(d_inc, outs[k][1], count=inc.shape[0], flags=capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE))
            if rep >= warmup:
                tg[k].append(g)
                ti[k].append(i)
    first = list(ctxs)[0]
    # records that differ from the first context's, per context: (grid, incoherent)
    diff = {k: [int((outs[first][j].view(-1, 32) != outs[k][j].view(-1, 32)).any(dim=1).sum()) for j in (0, 1)] for k in ctxs}
    return tg, ti, all(d == [0, 0] for d in diff.values()), diff


def bench(sc, a, stream, out):
    r = out[sc.name] = {"n_tris": int(sc.local.shape[0] if sc.inst is None else sc.inst["n_tris"].sum())}
    print(f"== {sc.name}: {r['n_tris']} triangles", flush=True)
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    sc.load(ctx, sc.local)
    frames = [sc.device_input(sc.frame(0.01, p)) for p in (0.0, 1.0)]
    dev, wall = [], []
    for k in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.refit(ctx, frames[k & 1])
        t = (time.perf_counter() - t0) * 1e3
        if k >= a.warmup:
            dev.append(ctx.stats()["last_build_ms"])
            wall.append(t)
    r["refit_device_ms"], r["refit_wall_ms"] = med(dev), med(wall)
    r["refit_device_ms_range"] = [min(dev), max(dev)]
    print(f"refit                 device {med(dev):8.3f} ms [{min(dev):.3f} .. {max(dev):.3f}]  wall {med(wall):8.3f} ms", flush=True)

    # rebuilds of the same frame (frames[1]'s geometry)
    world = sc.tris(sc.frame(0.01, 1.0))
    d_tris = torch.from_numpy(world.view(np.uint8).reshape(-1)).cuda()
    for label, kw in (("radix", {}), ("sah", {"sah": True})):
        dv, wl = [], []
        for k in range(a.warmup + min(a.repeats, 10)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.build_scene_device(d_tris, n_tris=world.shape[0], on_device=True, **kw)
            t = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                dv.append(ctx.stats()["last_build_ms"])
                wl.append(t)
        r[f"build_{label}_device_ms"], r[f"build_{label}_wall_ms"] = med(dv), med(wl)
        print(f"build_scene_device {label:5s} device {med(dv):8.3f} ms  wall {med(wl):8.3f} ms", flush=True)
    wl = []
    for k in range(1 if sc.name == "C5" else 3):
        t0 = time.perf_counter()
        nodes, prim_idx, _ = capi.bvh2_build(T.verts4_from_verts9(sc.world(sc.frame(0.01, 1.0))))
        ctx.upload_scene(world, nodes, prim_idx)
        wl.append((time.perf_counter() - t0) * 1e3)
    r["host_build_upload_wall_ms"] = med(wl)
    print(f"host SAH build + upload  wall {med(wl):8.1f} ms", flush=True)
    ctx.close()
    del d_tris, frames

    # identity refit against never refit
    ca, cb = capi.Context(0), capi.Context(0)
    for c in (ca, cb):
        c.set_stream(stream.cuda_stream)
        sc.load(c, sc.local)
    d0 = sc.device_input(sc.local)
    sc.refit(cb, d0)
    tg, ti, same, _ = trace_pair(sc, {"never": ca, "identity": cb}, stream, a.repeats, a.warmup)
    r["identity"] = {k: {"grid_ms": med(tg[k]), "grid_range": [min(tg[k]), max(tg[k])], "incoherent_ms": med(ti[k]),
                         "incoherent_range": [min(ti[k]), max(ti[k])]} for k in tg}
    r["identity"]["records_equal"] = same
    for k in tg:
        print(f"trace {k:8s} grid {sc.grid[0]}x{sc.grid[1]} {med(tg[k]):8.3f} ms [{min(tg[k]):.3f} .. {max(tg[k]):.3f}]   "
              f"2^22 incoherent {med(ti[k]):8.3f} ms [{min(ti[k]):.3f} .. {max(ti[k]):.3f}]", flush=True)
    print(f"identity refit records byte-equal: {same}", flush=True)

    # motion of growing amplitude: refit of the frame-0 tree against a fresh SAH build of the frame
    r["motion"] = []
    cf = capi.Context(0)
    cf.set_stream(stream.cuda_stream)
    for amp in AMPLITUDES:
        local = sc.frame(amp, 1.0)
        sc.refit(cb, sc.device_input(local))
        wt = sc.tris(local)
        cf.build_scene_device(torch.from_numpy(wt.view(np.uint8).reshape(-1)).cuda(), n_tris=wt.shape[0], on_device=True, sah=True)
        pair = {"refit": cb, "fresh_sah": cf}
        if amp == 0.0:
            pair["never"] = ca  # frame 0 itself: the scene never refit
        tg, ti, same, diff = trace_pair(sc, pair, stream, max(a.repeats // 4, 3), 1)
        row = dict(amplitude=amp, refit_grid_ms=med(tg["refit"]), fresh_grid_ms=med(tg["fresh_sah"]), refit_inc_ms=med(ti["refit"]),
                   fresh_inc_ms=med(ti["fresh_sah"]), records_equal=same, differing_records=diff)
        r["motion"].append(row)
        print(f"motion {amp:6.3f}: grid refit {row['refit_grid_ms']:8.3f} / fresh {row['fresh_grid_ms']:8.3f} ms ({row['refit_grid_ms'] / row['fresh_grid_ms']:.2f}x)"
              f"   incoherent refit {row['refit_inc_ms']:8.3f} / fresh {row['fresh_inc_ms']:8.3f} ms ({row['refit_inc_ms'] / row['fresh_inc_ms']:.2f}x)"
              f"   records equal {same}" + ("" if same else f" {diff}"), flush=True)
    for c in (ca, cb, cf):
        c.close()
    return same and r["identity"]["records_equal"] and all(m["records_equal"] for m in r["motion"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C5,room")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    stream = torch.cuda.current_stream()
    out, ok = {}, True
    for name in a.configs.split(","):
        ok &= bench(Scene(name), a, stream, out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"refit_bench": {k: {x: v[x] for x in ("n_tris", "refit_device_ms", "refit_wall_ms", "build_radix_device_ms",
                                                              "build_sah_device_ms", "host_build_upload_wall_ms")} for k, v in out.items()},
                      "records_equal": bool(ok)}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
