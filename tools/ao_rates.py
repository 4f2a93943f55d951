#!/usr/bin/env python3
"""Informational: G rays/s of ambient occlusion on the device (pt_render_ao) and of the early-exit occlusion search
(pt_occluded_rays).  Every leg is warmed up once, then timed `reps` times by device events; the median is recorded (one JSON line
each).
  (a) Cornell box 1024^2, 1 frame, K = 16, radius 1.0 and 1e20 -- pt_render_ao, its own event pair.  Rays = the primary rays
      (npix x frames) + K x sum(hits), known exactly from the counts.
  (b) the same AO composed from queries on the device: pt_camera_rays, the closest query, K directions per pixel made by torch,
      the occluded query of all of them, a miss's with tmax 0 (torch events around the whole composition, which never waits on the
      host; the same ray count formula).
  (c) the 10^6-triangle soup (scene.make_soup): 2^22 random rays, tmax 1.0 and 1e20, pt_occluded_rays against
      pt_intersect_rays(PT_QUERY_OCCLUDED), each its own event pair.
  (d) soup AO, 1024^2, 1 frame, K = 4, radius 1.0.
usage: python tools/ao_rates.py [reps] [out.jsonl]"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime in the process)

from oclpathtracer_amd import adl, scene  # noqa: E402
from oclpathtracer_amd.ao import AORenderer  # noqa: E402
from oclpathtracer_amd.query import RayCaster  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def fused(dev, tbuf, ntri, W, H, K, radius):
    """(median s, rays): pt_render_ao timed by its own event pair"""
    a = AORenderer(dev, tbuf, W, H, rays_per_sample=K, radius=radius, num_triangles=ntri, stripe_rows=1)
    ev = adl.SyncObject(dev)
    try:
        a.render(1, 0, sync=ev)
        dev.waitForCompletion()
        ts = []
        for _ in range(reps):
            a.render(1, 0, sync=ev)
            dev.waitForCompletion()
            ts.append(ev.getExecutionTimeNanoseconds() * 1e-9)
        hits = int(a.read_counts()[..., 1].astype(np.int64).sum())
    finally:
        ev.release()
        a.release()
    return median(ts), W * H + K * hits


def composed(rc, W, H, K, radius):
    """(median s, rays): the query composition, torch events around it.  Written without boolean indexing, so that nothing in
    the timed window waits on the host: every pixel gets K occlusion rays, and those of a pixel whose primary ray missed have
    tmax 0 (they search nothing and are not counted)."""
    def run():
        rays = rc.camera_rays(W, H, 0, as_tensor=True)
        hits = rc.closest(rays)
        hit = hits[:, 1].view(torch.int32) >= 0
        p = hits[:, 4:7]
        n = torch.where(hit[:, None], hits[:, 8:11], torch.tensor([0.0, 0.0, 1.0], device=hits.device))   # (a miss: any unit normal)
        d = torch.nn.functional.normalize(rays[:, 4:7], dim=1)
        n = torch.where(((n * d).sum(1) < 0)[:, None], n, -n)
        m = n.shape[0]
        axis = torch.where((n[:, 0].abs() > 0.001)[:, None], torch.tensor([0.0, 1.0, 0.0], device=n.device),
                           torch.tensor([1.0, 0.0, 0.0], device=n.device))
        t = torch.nn.functional.normalize(torch.cross(axis, n, dim=1), dim=1)
        s = torch.cross(n, t, dim=1)
        u1, u2 = torch.rand((2, m, K), device=n.device)
        phi, st, ct = 2 * math.pi * u1, u2.sqrt(), (1 - u2).sqrt()
        wi = (s[:, None] * (phi.cos() * st)[..., None] + t[:, None] * (phi.sin() * st)[..., None] + n[:, None] * ct[..., None]).reshape(-1, 3)
        occ = torch.empty((m * K, 8), dtype=torch.float32, device=n.device)
        occ[:, :3] = p.repeat_interleave(K, 0) + 0.01 * wi
        occ[:, 3] = (hit.to(torch.float32) * radius).repeat_interleave(K)
        occ[:, 4:7] = wi
        occ[:, 7] = 0.0
        return rc.occluded(occ), hit

    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, hit = run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return median(ts), W * H + K * int(hit.sum())


def query(rc, rays, early_exit):
    rc.occluded(rays, early_exit=early_exit)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        rc.occluded(rays, early_exit=early_exit)
        torch.cuda.synchronize()
        ts.append(rc._io._sync.getExecutionTimeNanoseconds() * 1e-9)   # the call's own event pair
    return median(ts)


assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    W = H = 1024
    tris, _ = scene.load_model()
    rc = RayCaster(dev, tris)
    for radius in (1.0, 1e20):
        t, rays = fused(dev, rc.tbuf, len(tris), W, H, 16, radius)
        emit({"leg": "a", "scene": "cornell", "what": "pt_render_ao 1024^2 x 1 frame", "K": 16, "radius": radius, "reps": reps,
              "median_ms": round(t * 1e3, 3), "rays": rays, "grays_per_s": round(rays / t / 1e9, 2)})
        t, rays = composed(rc, W, H, 16, radius)
        emit({"leg": "b", "scene": "cornell", "what": "camera rays + closest + torch directions + occluded", "K": 16, "radius": radius,
              "reps": reps, "median_ms": round(t * 1e3, 3), "rays": rays, "grays_per_s": round(rays / t / 1e9, 2)})
    rc.release()

    tris, _ = scene.make_soup()
    rc = RayCaster(dev, tris)
    pts = np.concatenate([tris["p1"][:, :3], tris["p2"][:, :3], tris["p3"][:, :3]])
    n = 1 << 22
    g = torch.Generator(device="cuda").manual_seed(2)
    lo, hi = torch.tensor(pts.min(0), device="cuda"), torch.tensor(pts.max(0), device="cuda")
    rr = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rr[:, :3] = lo + (hi - lo) * torch.rand((n, 3), generator=g, device="cuda")
    rr[:, 4:7] = torch.randn((n, 3), generator=g, device="cuda")
    for tmax in (1.0, 1e20):
        rr[:, 3] = tmax
        occ = float(rc.occluded(rr).float().mean())
        for early in (False, True):
            t = query(rc, rr, early)
            emit({"leg": "c", "scene": "soup", "what": "pt_occluded_rays" if early else "pt_intersect_rays(PT_QUERY_OCCLUDED)",
                  "tmax": tmax, "n": n, "occluded_fraction": round(occ, 4), "reps": reps, "median_ms": round(t * 1e3, 3),
                  "grays_per_s": round(n / t / 1e9, 3)})
    del rr
    t, rays = fused(dev, rc.tbuf, len(tris), W, H, 4, 1.0)
    emit({"leg": "d", "scene": "soup", "what": "pt_render_ao 1024^2 x 1 frame", "K": 4, "radius": 1.0, "reps": reps,
          "median_ms": round(t * 1e3, 3), "rays": rays, "grays_per_s": round(rays / t / 1e9, 3)})
    rc.release()
finally:
    adl.DeviceUtils.deallocate(dev)
