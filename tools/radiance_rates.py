#!/usr/bin/env python3
"""Informational: what the third sample start costs.  pt_radiance_rays over pt_camera_rays of a 1024^2 image (frame 0), 16 samples per
ray, B = 16, K = 1, MIS, lights by power, Roulette(3, 0.95), with moments -- one launch and one moments kernel -- beside
pt_render_indirect_rr plus pt_sample_moments for the same item count on the same prepared scene, in the same process: the Cornell box
(brute force, the table in LDS) and the 10^6-triangle soup with every 64th material emissive (LBVH).  Both legs are timed by DEVICE
EVENTS (the call's own pt_event: first kernel's start to last kernel's end; the render leg adds its two calls' events), warmed up
once at their shape, then run REPS times alternating radiance, render, render, radiance; the ratio is of the medians, and the spread of
each leg is printed beside it.  A ratio near 1 is the expectation: a 32-byte load stands where the camera arithmetic stood and no fold
runs.
usage: python tools/radiance_rates.py [--reps N] [--scene cornell|soup] [out.txt]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette  # noqa: E402
from oclpathtracer_amd.query import RayCaster  # noqa: E402

REPS = 3
if "--reps" in sys.argv:
    at = sys.argv.index("--reps")
    REPS = int(sys.argv[at + 1])
    del sys.argv[at: at + 2]
ONLY = None
if "--scene" in sys.argv:
    at = sys.argv.index("--scene")
    ONLY = sys.argv[at + 1]
    del sys.argv[at: at + 2]
out_path = sys.argv[1] if len(sys.argv) > 1 else None
W = H = 1024
SAMPLES, B = 16, 16
N = W * H


def emit(line):
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def legs(dev, name, tris, mats):
    lib = shim.load()
    ir = IndirectRenderer(dev, tris, mats, W, H, light_samples=1, max_bounces=B, mis=True, light_choice="power", roulette=Roulette(3, 0.95),
                          chunk_frames=SAMPLES, moments=True, stripe_rows=1)
    rc = ir.radiance_caster(workspace_bytes=12 * N * SAMPLES)
    qc = RayCaster(dev, ir.tbuf, num_triangles=ir.num_triangles)
    rb = adl.Buffer(dev, 32 * N, np.uint8)
    mb = adl.Buffer(dev, 56 * N, np.uint8)
    e1, e2 = adl.SyncObject(dev), adl.SyncObject(dev)
    try:
        shim.check(lib.pt_camera_rays(dev._h, None, W, H, 0, rb._h, None))
        p = shim.RadianceParams()
        p.num_rays, p.sample_count = N, SAMPLES
        p.num_triangles, p.num_materials, p.num_lights = ir.num_triangles, ir.num_materials, len(ir.lights)
        p.light_samples, p.max_bounces, p.reset = 1, B, 1

        def radiance():
            shim.check(lib.pt_radiance_rays(dev._h, ir.tbuf._h, ir.mbuf._h, ir._lights_h(), 1, ir.counts._h, ir.cdf._h, ir.tri_q._h, rb._h,
                                            rc.samples._h, mb._h, ctypes.byref(p), ctypes.byref(rc._rr), e1._h))
            e1.waitForCompletion()
            return e1.getExecutionTimeNanoseconds() * 1e-9

        def render():
            shim.check(ir._call(ir.params(SAMPLES, 0), e1))
            shim.check(lib.pt_sample_moments(dev._h, ir.samples._h, ir.mom._h, N, SAMPLES, 1, e2._h))
            e2.waitForCompletion()
            return (e1.getExecutionTimeNanoseconds() + e2.getExecutionTimeNanoseconds()) * 1e-9

        radiance()   # warm-up: the scene's preparation, both code objects
        render()
        t = {"radiance": [], "render": []}
        for _ in range(REPS):
            t["radiance"].append(radiance())
            t["render"].append(render())
            t["render"].append(render())
            t["radiance"].append(radiance())
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, what in (("radiance", "pt_radiance_rays (with moments)"), ("render", "pt_render_indirect_rr + pt_sample_moments")):
            emit("%-22s %-44s median %9.3f ms  %8.1f Msamples/s  min %9.3f max %9.3f ms over %d runs"
                 % (name, what, med[k] * 1e3, N * SAMPLES / med[k] / 1e6, min(t[k]) * 1e3, max(t[k]) * 1e3, len(t[k])))
        emit("%-22s radiance / render time: %.4f (the render leg's own spread: %+.2f%% .. %+.2f%% of its median)"
             % (name, med["radiance"] / med["render"], (min(t["render"]) / med["render"] - 1) * 100, (max(t["render"]) / med["render"] - 1) * 100))
    finally:
        for o in (e1, e2, rb, mb):
            o.release()
        qc.release()
        rc.release()
        ir.release()


assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    emit("%s; %d x %d rays (pt_camera_rays, frame 0), %d samples, B = %d, K = 1, MIS, lights by power, Roulette(3, 0.95); device events; "
         "one warm-up per leg, then %d x (radiance, render, render, radiance)" % (dev.getDeviceName(), W, H, SAMPLES, B, REPS))
    if ONLY in (None, "cornell"):
        legs(dev, "Cornell box", *scene.load_model())
    if ONLY in (None, "soup"):
        soup_t, soup_m = scene.make_soup()
        soup_m["emissive"][18::64, :3] = 30.0          # every 64th soup material emits (tools/indirect_rates.py's soup)
        legs(dev, "soup, %d triangles" % len(soup_t), soup_t, soup_m)
finally:
    adl.DeviceUtils.deallocate(dev)
