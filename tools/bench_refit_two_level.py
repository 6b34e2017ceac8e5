"""What a two-level refit costs and what it does to the trace.  Scenes: C5 as a two-level scene (64 meshes x
156 250 triangles, one instance each) and synth.room() (8 meshes, the boxes one mesh placed twice).  Frames come from synth.deform.
Per scene and BLAS form (host-built BLASes, device SAH BLASes):
  refit      mrt_refit_two_level_scene between two frames, mesh vertices on the device: device time (last_build_ms) and host wall
             time around the blocking call, median over --repeats after --warmup; also the wall time with host vertices;
  upload     mrt_upload_two_level_scene of the same frame with MRT_BUILD_BLAS_ON_DEVICE (radix, SAH) and with host BLASes (wall;
             C5 once), the alternatives a deforming mesh had before;
  identity   the grid (mrt_cast_grid) and 2^22 incoherent device-resident rays on a scene refit with its own vertices against the
             same scene never refit (two contexts, alternating casts, device events on one stream), records compared;
  motion     deformations of growing amplitude: trace times after a refit of the frame-0 trees against a fresh upload of the same
             frame in the same form, records compared.
    python tools/bench_refit_two_level.py [--configs C5,room] [--forms host,device_sah] [--repeats 20] [--warmup 3] [--json OUT]
    python tools/bench_refit_two_level.py --refits-only 10      (C5, device SAH BLASes: ten refits and nothing else, for a profiler)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
from messyerraytracer_amd import capi, synth  # noqa: E402
from bench_refit import ROOM_CAM, AMPLITUDES, med, trace_pair  # noqa: E402

FORMS = {"host": {}, "device_sah": {"blas_on_device": True, "sah": True}, "device_radix": {"blas_on_device": True}}


class Scene:
    def __init__(self, name):
        self.name = name
        if name == "C5":
            cfg = synth.CONFIGS["C5"]
            self.local, self.inst = synth.multi_mesh_instances(cfg["n_meshes"], cfg["tris_per_mesh"], cfg["s"], cfg["seed"])
            self.cam, self.grid = cfg, (2048, 2048)
        else:
            self.local, self.inst = synth.room()
            self.cam, self.grid = ROOM_CAM, ROOM_CAM["grid"]

    def frame(self, amplitude, phase):
        return synth.deform(self.local, amplitude, phase, seed=7)

    def load(self, ctx, local, form):
        ctx.upload_two_level_scene(local, self.inst, **FORMS[form])

    def refit(self, ctx, d_local):
        ctx.refit_two_level_scene(d_local, self.inst, n_mesh_tris=self.local.shape[0], on_device=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def refits(sc, ctx, frames, n, warmup):
    dv, wl = [], []
    for k in range(warmup + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.refit(ctx, frames[k & 1])
        t = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            dv.append(ctx.stats()["last_build_ms"])
            wl.append(t)
    return dv, wl


def bench(sc, form, a, stream, out):
    r = out[f"{sc.name}/{form}"] = {"n_tris": int(sc.local.shape[0]), "n_instances": int(sc.inst.shape[0])}
    print(f"== {sc.name}, {form} BLASes: {r['n_tris']} mesh triangles, {r['n_instances']} instances", flush=True)
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    sc.load(ctx, sc.local, form)
    host_frames = [sc.frame(0.01, p) for p in (0.0, 1.0)]
    frames = [dev(f) for f in host_frames]
    t0 = time.perf_counter()
    sc.refit(ctx, frames[0])
    r["first_refit_wall_ms"] = (time.perf_counter() - t0) * 1e3
    dv, wl = refits(sc, ctx, frames, a.repeats, a.warmup)
    r["refit_device_ms"], r["refit_wall_ms"], r["refit_device_ms_range"] = med(dv), med(wl), [min(dv), max(dv)]
    print(f"first refit (slot map, parents{', 8-wide layout' if form == 'host' else ''})  wall {r['first_refit_wall_ms']:8.3f} ms", flush=True)
    print(f"refit, device vertices  device {med(dv):8.3f} ms [{min(dv):.3f} .. {max(dv):.3f}]  wall {med(wl):8.3f} ms", flush=True)
    wl = []
    for k in range(a.warmup + min(a.repeats, 10)):
        t0 = time.perf_counter()
        ctx.refit_two_level_scene(host_frames[k & 1], sc.inst)
        if k >= a.warmup:
            wl.append((time.perf_counter() - t0) * 1e3)
    r["refit_host_vertices_wall_ms"] = med(wl)
    print(f"refit, host vertices    wall {med(wl):8.3f} ms", flush=True)
    # the re-uploads a deforming mesh cost before (every form, so the ratio is measured in the same run)
    for label in ("device_radix", "device_sah", "host"):
        dvu, wlu = [], []
        n = 1 if (label == "host" and sc.name == "C5") else a.warmup + min(a.repeats, 5)
        for k in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.upload_two_level_scene(host_frames[1], sc.inst, **FORMS[label])
            t = (time.perf_counter() - t0) * 1e3
            if n == 1 or k >= a.warmup:
                dvu.append(ctx.stats()["last_build_ms"] if label != "host" else float("nan"))  # (a host build sets no device time)
                wlu.append(t)
        r[f"upload_{label}_device_ms"], r[f"upload_{label}_wall_ms"] = med(dvu), med(wlu)
        print(f"upload {label:12s}     device {med(dvu):8.3f} ms  wall {med(wlu):8.3f} ms", flush=True)
    r["refit_over_device_sah_upload_wall"] = r["refit_wall_ms"] / r["upload_device_sah_wall_ms"]
    print(f"refit wall / device-SAH upload wall = {r['refit_over_device_sah_upload_wall']:.3f}", flush=True)
    ctx.close()
    del frames

    ca, cb = capi.Context(0), capi.Context(0)
    for c in (ca, cb):
        c.set_stream(stream.cuda_stream)
        sc.load(c, sc.local, form)
    sc.refit(cb, dev(sc.local))
    tg, ti, same, _ = trace_pair(sc, {"never": ca, "identity": cb}, stream, a.repeats, a.warmup)
    r["identity"] = {k: {"grid_ms": med(tg[k]), "grid_range": [min(tg[k]), max(tg[k])], "incoherent_ms": med(ti[k]),
                         "incoherent_range": [min(ti[k]), max(ti[k])]} for k in tg}
    r["identity"]["records_equal"] = same
    for k in tg:
        print(f"trace {k:8s} grid {sc.grid[0]}x{sc.grid[1]} {med(tg[k]):8.3f} ms [{min(tg[k]):.3f} .. {max(tg[k]):.3f}]   "
              f"2^22 incoherent {med(ti[k]):8.3f} ms [{min(ti[k]):.3f} .. {max(ti[k]):.3f}]", flush=True)
    print(f"identity refit records byte-equal: {same}", flush=True)

    r["motion"] = []
    cf = capi.Context(0)
    cf.set_stream(stream.cuda_stream)
    for amp in AMPLITUDES:
        local = sc.frame(amp, 1.0)
        sc.refit(cb, dev(local))
        sc.load(cf, local, form)
        tg, ti, same, diff = trace_pair(sc, {"refit": cb, "fresh": cf}, stream, max(a.repeats // 4, 3), 1)
        row = dict(amplitude=amp, refit_grid_ms=med(tg["refit"]), fresh_grid_ms=med(tg["fresh"]), refit_inc_ms=med(ti["refit"]),
                   fresh_inc_ms=med(ti["fresh"]), records_equal=same, differing_records=diff)
        r["motion"].append(row)
        print(f"motion {amp:6.3f}: grid refit {row['refit_grid_ms']:8.3f} / fresh {row['fresh_grid_ms']:8.3f} ms ({row['refit_grid_ms'] / row['fresh_grid_ms']:.2f}x)"
              f"   incoherent refit {row['refit_inc_ms']:8.3f} / fresh {row['fresh_inc_ms']:8.3f} ms ({row['refit_inc_ms'] / row['fresh_inc_ms']:.2f}x)"
              f"   records equal {same}" + ("" if same else f" {diff}"), flush=True)
    for c in (ca, cb, cf):
        c.close()
    return same and r["identity"]["records_equal"] and all(m["records_equal"] for m in r["motion"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C5,room")
    ap.add_argument("--forms", default="host,device_sah")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--refits-only", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.Stream()
    if a.refits_only:
        sc = Scene("C5")
        ctx = capi.Context(0)
        ctx.set_stream(stream.cuda_stream)
        sc.load(ctx, sc.local, "device_sah")
        frames = [dev(sc.frame(0.01, p)) for p in (0.0, 1.0)]
        sc.refit(ctx, frames[1])  # the first refit: slot map and parents
        dv, wl = refits(sc, ctx, frames, a.refits_only, 0)
        print(f"C5 device SAH: {a.refits_only} refits, device {med(dv):.3f} ms, wall {med(wl):.3f} ms", flush=True)
        ctx.close()
        return 0
    out, ok = {}, True
    for name in a.configs.split(","):
        sc = Scene(name)
        for form in a.forms.split(","):
            ok = bench(sc, form, a, stream, out) and ok
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print("records byte-equal everywhere:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
