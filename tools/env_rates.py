#!/usr/bin/env python3
"""Informational: what environment lighting (``environment=``, ``env_samples=Ke``) costs and buys ON THE DEVICE.  One process, one device.

SIZE^2 pixels, B = 16, K = 1, MIS, lights by power, roulette (3, 0.95), moments kept.

(a) The cost of the flag: the grey map (every texel 0.45, N = 64) with Ke = 0 through pt_render_indirect_env -- the parent's image bit
    for bit, made by the ENV kernels with their run-time lookup -- against the parent (pt_render_indirect_rr) on the Cornell box (brute
    force) and on the room of 64 emitters with filler (520 triangles, the LBVH).
(b) The cost and the gain of sampling: the Cornell room without ceiling and panel under the sun map (tests/env_scenes: four texels of
    5 000 on a sky of 0.45, N = 64) at Ke = 0, 1, 2, 4: the variance per sample (``noise().variance_per_sample``, pt_sample_moments), the
    time per sample, and their product relative to Ke = 0's: below 1 the estimator reaches a noise level sooner.
Every figure is taken against its baseline in the same process: the renders alternate REPS times after one warm-up round, timed by a
host clock around the call and the synchronise that ends it; medians with the spread (min .. max).
No figure is gated.  usage: python tools/env_rates.py [rates.txt] [--size 1024] [--frames 16] [--reps 5]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from env_scenes import env_map, env_scene  # noqa: E402
from oclpathtracer_amd import adl, scene  # noqa: E402
from oclpathtracer_amd.environment import Environment  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette  # noqa: E402
from ris_scenes import many_lights_lbvh  # noqa: E402

args = sys.argv[1:]


def option(name, default):
    if name in args:
        at = args.index(name)
        value = args[at + 1]
        del args[at: at + 2]
        return value
    return default


SIZE = int(option("--size", 1024))
FRAMES = int(option("--frames", 16))
REPS = int(option("--reps", 5))
KES = (0, 1, 2, 4)
out_path = (args + [None])[0]
if out_path:
    open(out_path, "w").close()   # a run is one record: a second run replaces the first


def emit(line):
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def spread(values, fmt="%.1f"):
    v = np.asarray(values, np.float64)
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (float(np.median(v)), float(v.min()), float(v.max()))


def alternate(dev, r, settings):
    """{key: (times of REPS runs, variance per sample, rejected)}: the settings rendered in turn, REPS times after one warm-up round"""
    times = {k: [] for k, _ in settings}
    var = {}
    for rep in range(REPS + 1):
        for key, (env, ke) in settings:
            r.set_environment(env, ke)
            dev.waitForCompletion()
            t0 = time.perf_counter()
            r.render(FRAMES, 0)
            dev.waitForCompletion()
            dt = time.perf_counter() - t0
            if rep:
                times[key].append(dt)
            else:
                n = r.noise()
                var[key] = (n.variance_per_sample, n.rejected)
    return {k: (times[k], var[k][0], var[k][1]) for k in times}


assert adl.init()
dev = adl.DeviceUtils.allocate()
grey = Environment(env_map("grey:64"))
sun = Environment(env_map("sun"))
nsamples = SIZE * SIZE * FRAMES
kw = dict(max_bounces=16, light_samples=1, mis=True, light_choice="power", roulette=Roulette(3, 0.95), stripe_rows=1, moments=True,
          chunk_frames=FRAMES)
try:
    emit("%s; %d^2 pixels, %d frames per run, MIS, lights by power, roulette (3, 0.95), B = 16, K = 1; medians of %d alternating runs after "
         "one warm-up round, (min .. max)" % (dev.getDeviceName(), SIZE, FRAMES, REPS))
    emit("(a) the cost of the flag: the grey map with Ke = 0 against the parent")
    for what, (tris, mats) in (("Cornell box, brute force (36 triangles)", scene.load_model()),
                               ("64 emitters with filler, LBVH (520 triangles)", many_lights_lbvh())):
        r = IndirectRenderer(dev, tris, mats, SIZE, SIZE, **kw)
        try:
            got = alternate(dev, r, (("parent", (None, 0)), ("env", (grey, 0))))
            tp, te = float(np.median(got["parent"][0])), float(np.median(got["env"][0]))
            emit("  %s" % what)
            emit("    pt_render_indirect_rr     %s Msamples/s" % spread([nsamples / x * 1e-6 for x in got["parent"][0]]))
            emit("    pt_render_indirect_env    %s Msamples/s; time per sample %.3f of the parent's; variance per sample %.6g against %.6g"
                 % (spread([nsamples / x * 1e-6 for x in got["env"][0]]), te / tp, got["env"][1], got["parent"][1]))
        finally:
            r.release()
    emit("(b) the open room (no ceiling, no panel: 32 triangles) under the sun map")
    tris, mats, lights, cam = env_scene("open")
    r = IndirectRenderer(dev, np.array(tris), np.array(mats), SIZE, SIZE, lights=lights, camera=cam, **kw)
    try:
        got = alternate(dev, r, tuple(("Ke = %d" % ke, (sun, ke)) for ke in KES))
        t0, v0 = float(np.median(got["Ke = 0"][0])), got["Ke = 0"][1]
        for key, (times, v, rejected) in got.items():
            t = float(np.median(times))
            emit("  %-8s %s Msamples/s; time per sample %.3f of Ke = 0's; variance per sample %.6g (%.4f of Ke = 0's; %d rejected); variance x time %.4f"
                 % (key, spread([nsamples / x * 1e-6 for x in times]), t / t0, v, v / v0, rejected, v / v0 * t / t0))
        best = min(got, key=lambda k: got[k][1] * float(np.median(got[k][0])))
        emit("  smallest variance x time at %s" % best)
    finally:
        r.release()
finally:
    grey.release()
    sun.release()
    adl.DeviceUtils.deallocate(dev)
