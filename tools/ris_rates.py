#!/usr/bin/env python3
"""Informational: what resampled light sampling (``candidates=M``) costs and buys ON THE DEVICE.  One process, one device.

Scenes: the room of 64 equal emitters (tests/ris_scenes.many_lights: 100 triangles, the brute-force refilling kernel), its LBVH form
(520 triangles), and the Cornell box (two equal emitters: the gain should be small).  SIZE^2 pixels, B = 16, K = 1, MIS, lights by
power, roulette (3, 0.95), moments kept.

Per scene the parent (pt_render_indirect_rr) and M in {1, 2, 4, 8, 16, 32} through pt_render_indirect_ris -- M = 1 is forced through
the RIS kernel (``set_candidates(1, through_ris=True)``), which a renderer with ``candidates=1`` does not use -- render FRAMES frames
from frame 0, timed by a host clock around the call and the synchronise that ends it, alternating REPS times after one warm-up round; samples per second with the spread (min ..
max).  The variance per sample is ``noise().variance_per_sample`` of those frames (pt_sample_moments); the efficiency figure is
variance x time per sample relative to the parent's: below 1 the estimator reaches a noise level sooner.
No figure is gated.  usage: python tools/ris_rates.py [rates.txt] [--size 1024] [--frames 16] [--reps 5]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette  # noqa: E402
from ris_scenes import many_lights, many_lights_lbvh  # noqa: E402

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
MS = (1, 2, 4, 8, 16, 32)
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


assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    emit("%s; %d^2 pixels, %d frames per run, MIS, lights by power, roulette (3, 0.95), B = 16, K = 1; medians of %d alternating runs after "
         "one warm-up round, (min .. max)" % (dev.getDeviceName(), SIZE, FRAMES, REPS))
    for what, (tris, mats) in (("64 equal emitters, brute force (100 triangles)", many_lights()),
                               ("64 equal emitters, LBVH (520 triangles)", many_lights_lbvh()),
                               ("Cornell box, two equal emitters (36 triangles)", scene.load_model())):
        r = IndirectRenderer(dev, tris, mats, SIZE, SIZE, max_bounces=16, light_samples=1, mis=True, light_choice="power", roulette=Roulette(3, 0.95),
                             stripe_rows=1, moments=True, chunk_frames=FRAMES)
        try:
            times = {M: [] for M in (0,) + MS}     # 0: the parent
            var = {}
            for rep in range(REPS + 1):
                for M in times:
                    r.set_candidates(max(M, 1), through_ris=M > 0)
                    dev.waitForCompletion()
                    t0 = time.perf_counter()
                    r.render(FRAMES, 0)
                    dev.waitForCompletion()
                    dt = time.perf_counter() - t0
                    if rep:
                        times[M].append(dt)
                    else:
                        n = r.noise()
                        var[M] = (n.variance_per_sample, n.rejected)
            emit(what)
            nsamples = SIZE * SIZE * FRAMES
            base_t, base_v = float(np.median(times[0])), var[0][0]
            for M in times:
                t = float(np.median(times[M]))
                emit("  %-22s %s Msamples/s; time per sample %.3f of the parent's; variance per sample %.6g (%.3f of the parent's; %d rejected); "
                     "variance x time %.3f" % ("pt_render_indirect_rr" if M == 0 else "M = %d" % M, spread([nsamples / x * 1e-6 for x in times[M]]),
                                               t / base_t, var[M][0], var[M][0] / base_v, var[M][1], var[M][0] / base_v * t / base_t))
            best = min(MS, key=lambda M: var[M][0] * float(np.median(times[M])))
            emit("  smallest variance x time at M = %d" % best)
        finally:
            r.release()
finally:
    adl.DeviceUtils.deallocate(dev)
