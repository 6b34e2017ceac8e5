"""What moving the instances of a two-level scene costs with the top level built on the host and on the device.
Scene: synth.many_instances(n) -- 4 meshes of 24 triangles placed n times, overlapping, every 64th instance an exact duplicate.
Per instance count (64, 8 192, 65 536, 262 144 by default):
  update   host mrt_update_instances (wall) against mrt_update_instances_device in each tree form (radix, PLOC, SAH), from host and
           from device instances: host wall time around the blocking call and device time (last_build_ms), median and [min .. max]
           over --repeats after --warmup, two placements alternating;
  trace    a 1280x960 grid (mrt_cast_grid) and 2^20 incoherent device-resident rays over the top level each path built, trace time
           (last_trace_ms) median over --repeats, relative to the host top level's; the records of every form compared with the host's.
    python tools/bench_instances_device.py [--counts 64,8192,65536,262144] [--repeats 20] [--warmup 3] [--json OUT]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from messyerraytracer_amd import capi, synth, types as T  # noqa: E402

FORMS = ("radix", "ploc", "sah")
CAM = ((0.0, 0.0, -12.0), (0.0, 0.0, 1.0), 50.0)
GRID = (1280, 960)
N_INC = 1 << 20


def med(v):
    return float(np.median(v)) if len(v) else float("nan")


def spread(v):
    return [float(min(v)), float(max(v))] if len(v) else []


def moved(inst, step):
    """a placement per step: every instance turned about z and shifted (exact duplicates stay duplicates)"""
    n = inst.shape[0]
    a = np.float64(0.1 + 0.05 * step)
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    m = inst.copy()
    m["basis"] = np.einsum("ij,njk->nik", rot, inst["basis"].reshape(n, 3, 3).astype(np.float64)).astype(np.float32).reshape(n, 9)
    m["origin"] += np.float32([0.05 * step, -0.03 * step, 0.02 * step])
    return m


def timed(fn, ctx, placements, repeats, warmup, device_time=True):
    wall, dev = [], []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        fn(placements[k & 1])
        t = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            wall.append(t)
            if device_time:
                dev.append(ctx.stats()["last_build_ms"])
    return wall, dev


def traces(ctx, d_rays, d_hits, repeats, warmup):
    cam = capi.camera_look(CAM[0], CAM[1], GRID[0], GRID[1], CAM[2])
    tg, ti = [], []
    for k in range(warmup + repeats):
        ctx.cast_grid(cam, GRID[0], GRID[1], hits=d_hits, flags=capi.FLAG_HITS_ON_DEVICE)
        if k >= warmup:
            tg.append(ctx.stats()["last_trace_ms"])
    grid = np.zeros(GRID[0] * GRID[1], dtype=T.HIT32)
    ctx.d2h(grid, d_hits)
    for k in range(warmup + repeats):
        ctx.cast(d_rays, d_hits, count=N_INC, flags=capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE)
        if k >= warmup:
            ti.append(ctx.stats()["last_trace_ms"])
    inc = np.zeros(N_INC, dtype=T.HIT32)
    ctx.d2h(inc, d_hits)
    return tg, ti, grid.tobytes() + inc.tobytes()


def bench(n, a, out):
    local, inst = synth.many_instances(n)
    place = [moved(inst, 1), moved(inst, 2)]
    r = out[str(n)] = {"n_instances": n, "n_mesh_tris": int(local.shape[0])}
    print(f"== {n} instances ({local.shape[0]} mesh triangles)", flush=True)
    ctx = capi.Context(0)
    ctx.upload_two_level_scene(local, inst)
    d_place = []
    for p in place:
        d = ctx.device_alloc(p.nbytes)
        ctx.h2d(d, p)
        d_place.append(d)
    d_rays, d_hits = ctx.device_alloc(N_INC * 32), ctx.device_alloc(max(N_INC, GRID[0] * GRID[1]) * 32)
    ctx.h2d(d_rays, synth.incoherent_rays(N_INC, 21))
    try:
        wall, _ = timed(ctx.update_instances, ctx, place, a.repeats, a.warmup, device_time=False)
        r["host"] = {"wall_ms": med(wall), "wall_range": spread(wall), "device_ms": None}
        print(f"host update_instances              wall {med(wall):9.3f} ms [{min(wall):.3f} .. {max(wall):.3f}]   device: not measured", flush=True)
        for form in FORMS:
            for src in ("host", "device"):
                if src == "host":
                    fn = lambda p, f=form: ctx.update_instances_device(p, form=f)  # noqa: E731
                    ps = place
                else:
                    fn = lambda p, f=form: ctx.update_instances_device(p, on_device=True, form=f, n_instances=n)  # noqa: E731
                    ps = d_place
                wall, dev = timed(fn, ctx, ps, a.repeats, a.warmup)
                r[f"{form}/{src}"] = {"wall_ms": med(wall), "wall_range": spread(wall), "device_ms": med(dev), "device_range": spread(dev)}
                print(f"device {form:5s}, {src:6s} instances      wall {med(wall):9.3f} ms [{min(wall):.3f} .. {max(wall):.3f}]"
                      f"   device {med(dev):8.3f} ms [{min(dev):.3f} .. {max(dev):.3f}]", flush=True)
        # trace over each top level (the same placement), relative to the host's
        ctx.update_instances(place[0])
        tg0, ti0, rec0 = traces(ctx, d_rays, d_hits, a.repeats, a.warmup)
        r["trace_host"] = {"grid_ms": med(tg0), "grid_range": spread(tg0), "incoherent_ms": med(ti0), "incoherent_range": spread(ti0)}
        print(f"trace, host TLAS          grid {med(tg0):8.3f} ms   2^20 incoherent {med(ti0):8.3f} ms", flush=True)
        for form in FORMS:
            ctx.update_instances_device(place[0], form=form)
            tg, ti, rec = traces(ctx, d_rays, d_hits, a.repeats, a.warmup)
            r[f"trace_{form}"] = {"grid_ms": med(tg), "grid_range": spread(tg), "incoherent_ms": med(ti), "incoherent_range": spread(ti),
                                  "grid_rel": med(tg) / med(tg0), "incoherent_rel": med(ti) / med(ti0), "records_equal": rec == rec0}
            print(f"trace, device {form:5s} TLAS  grid {med(tg):8.3f} ms ({med(tg) / med(tg0):.3f} x)   2^20 incoherent {med(ti):8.3f} ms "
                  f"({med(ti) / med(ti0):.3f} x)   records equal: {rec == rec0}", flush=True)
    finally:
        for d in d_place + [d_rays, d_hits]:
            ctx.device_free(d)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="64,8192,65536,262144")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = {}
    for n in [int(x) for x in a.counts.split(",")]:
        bench(n, a, out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
