#!/usr/bin/env python3
"""Informational: Mrays/s of the batched ray queries (pt_intersect_rays) beside the renderer's own rays/s on the same scene.

Cases (one JSON line each, median of `reps` timed calls after a warm-up; the query's time is its kernel's, from the event
pt_intersect_rays records around it; rays and results are device tensors, so no transfer is timed; the renderer's time is its
trace kernels' device time, the union of their launches' event intervals -- the wall time is recorded beside it):
  cornell  2^24 random rays   closest / occluded      renderer: configs[2] (1024^2 x 256 spp, depth 16), PT_STAT_RAYS / render time
  soup     1024^2 camera rays closest                 renderer: the configs[4] scene, 1024^2 x 8 spp
  soup     2^22 random rays   closest / occluded
Random rays start inside the scene's bounds with normally distributed directions.
usage: python tools/query_rates.py [reps] [out.jsonl]"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime in the process)

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.query import RayCaster  # noqa: E402
from oclpathtracer_amd.render import Renderer  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def random_rays(n, lo, hi, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    lo_t = torch.tensor(lo, dtype=torch.float32, device="cuda")
    hi_t = torch.tensor(hi, dtype=torch.float32, device="cuda")
    r[:, :3] = lo_t + (hi_t - lo_t) * torch.rand((n, 3), generator=g, device="cuda")
    r[:, 3] = 1e20
    r[:, 4:7] = torch.randn((n, 3), generator=g, device="cuda")
    r[:, 7] = 0.0
    return r


def time_query(rc, rays, mode):
    fn = rc.closest if mode == "closest" else rc.occluded
    fn(rays)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        fn(rays)
        ts.append(rc._io._sync.getExecutionTimeNanoseconds() * 1e-9)   # the query's own event pair
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def time_render(dev, tris, mats, W, H, spp):
    """The renderer's time as the query's is taken -- on the device, its own kernels only: the union of its trace launches'
    event intervals (pt_profile_query_union, PT_PROF_TRACE; no fold, no host).  Returns (median trace ms, median wall ms, rays)."""
    lib = shim.load()
    r = Renderer(dev, tris, mats, W, H, want_stats=True)
    r.render(spp, frame_begin=0)
    dev.waitForCompletion()
    shim.check(lib.pt_profile_enable(dev._h, 1))
    ts, walls, rays = [], [], 0
    for _ in range(reps):
        r.stats.write(np.zeros(shim.PT_STAT_WORDS, np.uint64), shim.PT_STAT_WORDS)
        dev.waitForCompletion()
        shim.check(lib.pt_profile_reset(dev._h))
        t0 = time.perf_counter()
        r.render(spp, frame_begin=0)
        dev.waitForCompletion()
        walls.append(time.perf_counter() - t0)
        u = ctypes.c_double(0.0)
        shim.check(lib.pt_profile_query_union(dev._h, shim.PT_PROF_TRACE, ctypes.byref(u)))
        ts.append(u.value * 1e-3)
        rays = int(r.read_stats_raw()[shim.PT_STAT_RAYS])
    shim.check(lib.pt_profile_enable(dev._h, 0))
    r.release()
    ts.sort()
    walls.sort()
    return ts[len(ts) // 2], walls[len(walls) // 2], rays


def case(scene_name, what, n, med, best, extra=None):
    rec = {"scene": scene_name, "rays": what, "n": n, "reps": reps, "median_ms": round(med * 1e3, 3), "min_ms": round(best * 1e3, 3),
           "mrays_per_s": round(n / med / 1e6, 1)}
    rec.update(extra or {})
    emit(rec)


assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    # ---- Cornell box ----------------------------------------------------------------------------------------------------
    tris, mats = scene.load_model()
    med, wall, rays = time_render(dev, tris, mats, 1024, 1024, 256)
    emit({"scene": "cornell", "renderer": "configs[2]: 1024^2 x 256 spp, depth 16", "reps": reps, "trace_ms": round(med * 1e3, 3),
          "wall_ms": round(wall * 1e3, 3), "rays": rays, "mrays_per_s": round(rays / med / 1e6, 1)})
    pts = np.concatenate([tris["p1"][:, :3], tris["p2"][:, :3], tris["p3"][:, :3]])
    rc = RayCaster(dev, tris)
    rr = random_rays(1 << 24, pts.min(0).tolist(), pts.max(0).tolist(), 1)
    for mode in ("closest", "occluded"):
        m, b = time_query(rc, rr, mode)
        case("cornell", "random", 1 << 24, m, b, {"query": mode})
    del rr
    rc.release()
    # ---- configs[4] soup --------------------------------------------------------------------------------------------------
    tris, mats = scene.make_soup()
    med, wall, rays = time_render(dev, tris, mats, 1024, 1024, 8)
    emit({"scene": "soup", "renderer": "configs[4] scene, 1024^2 x 8 spp, depth 16", "reps": reps, "trace_ms": round(med * 1e3, 3),
          "wall_ms": round(wall * 1e3, 3), "rays": rays, "mrays_per_s": round(rays / med / 1e6, 1)})
    rc = RayCaster(dev, tris)
    cam = rc.camera_rays(1024, 1024, 0, as_tensor=True)
    m, b = time_query(rc, cam, "closest")
    case("soup", "camera 1024^2", 1 << 20, m, b, {"query": "closest"})
    del cam
    pts = np.concatenate([tris["p1"][:, :3], tris["p2"][:, :3], tris["p3"][:, :3]])
    rr = random_rays(1 << 22, pts.min(0).tolist(), pts.max(0).tolist(), 2)
    for mode in ("closest", "occluded"):
        m, b = time_query(rc, rr, mode)
        case("soup", "random", 1 << 22, m, b, {"query": mode})
    rc.release()
finally:
    adl.DeviceUtils.deallocate(dev)
