#!/usr/bin/env python3
"""Informational: ns per sample of the first-hit feature buffers (pt_render_features) against the library's other route to the same
data, and against ambient occlusion's primary ray.  Every leg is warmed up once, then timed `reps` times by device events; the median
and the spread (max - min) / median are recorded, one JSON line each.  Per scene -- the Cornell box and the configs[4] soup
(scene.make_soup), 1024^2, `frames` frames:
  (y) the yardstick: pt_camera_rays + pt_intersect_rays(PT_QUERY_CLOSEST), one pair of calls per frame, torch events around the frames.
      Timed TWICE, at the start and at the end of the scene's legs: the difference of the two medians over their mean is the same-box
      run-to-run spread the comparison is read against;
  (f) pt_render_features, all four outputs, one call of `frames` frames, its own event pair;
  (d) pt_render_features, depth only;
  (a) pt_render_ao with K = 1 and a radius of 1e-30: the primary search, the hit's surface and one occlusion ray that searches next
      to nothing -- what a lit renderer pays for its first vertex.
usage: python tools/feature_rates.py [reps] [frames] [out.jsonl]"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime in the process)

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.ao import AORenderer  # noqa: E402
from oclpathtracer_amd.query import RayCaster  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 4
out_path = sys.argv[3] if len(sys.argv) > 3 else None
W = H = 1024


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, (ts[-1] - ts[0]) / med


def yardstick(rc):
    def run():
        for frame in range(frames):
            rc.closest(rc.camera_rays(W, H, frame, as_tensor=True))

    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return stats(ts)


def features(dev, lib, tbuf, mbuf, ntri, nmat, which):
    n = 3 * W * H * frames
    bufs = [adl.Buffer(dev, n, np.float32) if w else None for w in which]
    ev = adl.SyncObject(dev)
    p = shim.FeatureParams()
    p.width, p.height, p.frame_begin, p.frame_count = W, H, 0, frames
    p.num_triangles, p.num_materials, p.stripe_rows, p.n_ranks, p.rank = ntri, nmat, 1, 1, 0
    try:
        ts = []
        for k in range(reps + 1):
            shim.check(lib.pt_render_features(dev._h, tbuf._h, mbuf._h, *[b._h if b else None for b in bufs], ctypes.byref(p), None, ev._h))
            dev.waitForCompletion()
            if k:
                ts.append(ev.getExecutionTimeNanoseconds() * 1e-9)
    finally:
        ev.release()
        for b in bufs:
            if b:
                b.release()
    return stats(ts)


def ao_primary(dev, tbuf, ntri):
    a = AORenderer(dev, tbuf, W, H, rays_per_sample=1, radius=1e-30, num_triangles=ntri, stripe_rows=1)
    ev = adl.SyncObject(dev)
    try:
        ts = []
        for k in range(reps + 1):
            a.render(frames, 0, sync=ev)
            dev.waitForCompletion()
            if k:
                ts.append(ev.getExecutionTimeNanoseconds() * 1e-9)
    finally:
        ev.release()
        a.release()
    return stats(ts)


assert adl.init()
dev = adl.DeviceUtils.allocate()
lib = shim.load()
samples = W * H * frames
try:
    for name, (tris, mats) in (("cornell", scene.load_model()), ("soup", scene.make_soup())):
        rc = RayCaster(dev, tris)
        mbuf = adl.Buffer(dev, len(mats), scene.MATERIAL_DTYPE)
        mbuf.write(np.ascontiguousarray(mats), len(mats))
        try:
            def leg(tag, what, med, spread, **more):
                emit(dict({"leg": tag, "scene": name, "triangles": len(tris), "what": what, "frames": frames, "reps": reps,
                           "median_ms": round(med * 1e3, 4), "spread": round(spread, 4), "ns_per_sample": round(med / samples * 1e9, 4)}, **more))

            y0, s0 = yardstick(rc)
            leg("y", "pt_camera_rays + pt_intersect_rays per frame (first run)", y0, s0)
            f4, sf = features(dev, lib, rc.tbuf, mbuf, len(tris), len(mats), (1, 1, 1, 1))
            fd, sd = features(dev, lib, rc.tbuf, mbuf, len(tris), len(mats), (0, 0, 1, 0))
            ao, sa = ao_primary(dev, rc.tbuf, len(tris))
            y1, s1 = yardstick(rc)
            leg("y", "pt_camera_rays + pt_intersect_rays per frame (second run)", y1, s1)
            y = 0.5 * (y0 + y1)
            run_to_run = abs(y1 - y0) / y
            leg("f", "pt_render_features, four outputs", f4, sf, over_yardstick=round(f4 / y, 4), over_ao_primary=round(f4 / ao, 4))
            leg("d", "pt_render_features, depth only", fd, sd, over_yardstick=round(fd / y, 4), over_ao_primary=round(fd / ao, 4))
            leg("a", "pt_render_ao, K = 1, radius 1e-30", ao, sa)
            emit({"scene": name, "yardstick_run_to_run": round(run_to_run, 4), "features_no_slower_than_yardstick_plus_spread": bool(f4 <= y * (1 + run_to_run)),
                  "depth_no_slower_than_yardstick_plus_spread": bool(fd <= y * (1 + run_to_run))})
        finally:
            mbuf.release()
            rc.release()
finally:
    adl.DeviceUtils.deallocate(dev)
