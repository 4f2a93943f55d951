#!/usr/bin/env python3
"""Informational: the estimators' variance per sample ON THE DEVICE, from the renderers' own moments (``moments=True``:
pt_sample_moments after every call, pt_moments_resolve for the figures), and what keeping the moments costs.  One process, one device.

Variance (first output file): ``variance_per_sample`` -- the mean over pixels and channels of the unbiased variance of one sample's
linear radiance --, ``rejected`` and the ratios, each at 256^2 and 1024^2 over 256 frames:
  * Cornell box, IndirectRenderer B = 16, K = 1 and 4: plain against MIS;
  * the unequal-lights room of tests/power_scenes.py, B = 16, K = 1: uniform against power, without and with MIS;
  * the 10^6-triangle soup with every 64th material emissive, DirectRenderer K = 4: uniform against power.
Rates (second output file): every one of those renders timed with and without moments, alternating in the same process (a host clock
around the enqueue and the synchronise that ends it; the first run of each pair is a warm-up and is not counted), and
pt_sample_moments alone by device events on a full workspace against the time its bytes need at 6.29 TB/s (the samples it reads, 12 B
each, plus the 56-byte record read and written per pixel).
With --roulette the legs are Russian roulette's instead (IndirectRenderer(roulette=Roulette(3, 0.95))): Cornell box, B = 16, K = 1 and 4,
plain and MIS, without against with roulette -- the variance per sample, its ratio, and the efficiency 1 / (variance per sample x time
per sample) of both from the timed renders without moments.
No figure is gated.  usage: python tools/variance_rates.py [variance.txt [rates.txt]] [--frames N] [--sizes 256,1024] [--roulette]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.direct import DirectRenderer  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # the measured copy bandwidth the kernels of this project are held against
args = sys.argv[1:]


def option(name, default):
    if name in args:
        at = args.index(name)
        value = args[at + 1]
        del args[at: at + 2]
        return value
    return default


ROULETTE = "--roulette" in args
if ROULETTE:
    args.remove("--roulette")
FRAMES = int(option("--frames", 256))
SIZES = [int(s) for s in str(option("--sizes", "256,1024")).split(",")]
REPS = 3
var_path, rate_path = (args + [None, None])[:2]


def emit(path, line):
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def timed(dev, run):
    dev.waitForCompletion()
    t0 = time.perf_counter()
    run()
    dev.waitForCompletion()
    return time.perf_counter() - t0


def leg(dev, name, make, size):
    """one estimator at one size: its noise figures over FRAMES frames, and the render's time with and without moments"""
    with_m, without = make(size, True), make(size, False)
    try:
        tm, tp = [], []
        for rep in range(REPS + 1):            # alternating; pair 0 warms both up
            a = timed(dev, lambda: without.render(FRAMES, 0))
            b = timed(dev, lambda: with_m.render(FRAMES, 0))
            if rep:
                tp.append(a)
                tm.append(b)
        fig = with_m.noise()
        n = size * size * FRAMES
        a, b = float(np.median(tp)), float(np.median(tm))
        emit(rate_path, "%-58s %5d^2  plain %9.3f ms (%8.1f Msamples/s)  moments %9.3f ms (%8.1f)  ratio %.3f  [%d chunks of %d frames]"
             % (name, size, a * 1e3, n / a / 1e6, b * 1e3, n / b / 1e6, b / a, -(-FRAMES // with_m.chunk_frames), with_m.chunk_frames))
        emit(var_path, "%-58s %5d^2  variance_per_sample %-12.6g relative_error %-10.4g pixels %d samples %d rejected %d"
             % (name, size, fig.variance_per_sample, fig.relative_error, fig.pixels, fig.samples, fig.rejected))
        leg.seconds_per_sample = a / n       # (of the render without moments: what the efficiency figures use)
        return fig
    finally:
        with_m.release()
        without.release()


def ratio(what, a, b, size):
    emit(var_path, "%-58s %5d^2  ratio %.4g" % (what, size, a.variance_per_sample / b.variance_per_sample))


def accumulate_alone(dev, size):
    """pt_sample_moments by device events on the default workspace of a size x size image, reset = 0, the median of 9 after a warm-up"""
    tris, mats = scene.load_model()
    r = DirectRenderer(dev, tris, mats, size, size, stripe_rows=1, moments=True)
    ev = adl.SyncObject(dev)
    try:
        r.render(r.chunk_frames, 0)            # the workspace holds real samples, the records real sums
        ns = []
        for rep in range(10):
            shim.check(r._lib.pt_sample_moments(dev._h, r.samples._h, r.mom._h, r.local_pixels, r.chunk_frames, 0, ev._h))
            ev.waitForCompletion()
            ns.append(ev.getExecutionTimeNanoseconds())
        t = float(np.median(ns[1:])) * 1e-9
        nbytes = r.local_pixels * (12 * r.chunk_frames + 2 * 56)
        emit(rate_path, "pt_sample_moments %5d^2 x %2d frames: %9.1f us by events (median of 9); %.1f MB (12 B per sample + the 56-byte record read and "
             "written) need %7.1f us at 6.29 TB/s: %.2f of that rate" % (size, r.chunk_frames, t * 1e6, nbytes / 1e6, nbytes / HBM_BYTES_PER_S * 1e6,
                                                                         nbytes / HBM_BYTES_PER_S / t))
    finally:
        ev.release()
        r.release()


assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    head = "%s; %d frames per figure; IndirectRenderer at B = 16 unless stated" % (dev.getDeviceName(), FRAMES)
    emit(var_path, head)
    emit(rate_path, head + "; medians of %d alternating runs after one warm-up pair" % REPS)
    tris, mats = scene.load_model()
    if ROULETTE:
        from oclpathtracer_amd.indirect import Roulette

        for size in SIZES:
            for K in (1, 4):
                for mis in (False, True):
                    fig, eff = {}, {}
                    for rr in (None, Roulette(3, 0.95)):
                        name = "Cornell box K = %d %s, %s" % (K, "MIS" if mis else "plain", "roulette from 3, at most 0.95" if rr else "no roulette")
                        fig[rr] = leg(dev, name, lambda s, m: IndirectRenderer(dev, tris, mats, s, s, max_bounces=16, light_samples=K, mis=mis, roulette=rr,
                                                                               stripe_rows=1, moments=m), size)
                        eff[rr] = 1.0 / (fig[rr].variance_per_sample * leg.seconds_per_sample)
                        emit(var_path, "%-58s %5d^2  efficiency %.5g per second" % (name, size, eff[rr]))
                    rr = Roulette(3, 0.95)
                    ratio("Cornell box K = %d %s roulette / none" % (K, "MIS" if mis else "plain"), fig[rr], fig[None], size)
                    emit(var_path, "%-58s %5d^2  efficiency ratio %.4g" % ("Cornell box K = %d %s roulette / none" % (K, "MIS" if mis else "plain"), size,
                                                                            eff[rr] / eff[None]))
        sys.exit(0)
    for size in SIZES:
        for K in (1, 4):
            fig = {}
            for mis in (False, True):
                fig[mis] = leg(dev, "Cornell box K = %d %s" % (K, "MIS" if mis else "plain"),
                               lambda s, m: IndirectRenderer(dev, tris, mats, s, s, max_bounces=16, light_samples=K, mis=mis, stripe_rows=1, moments=m), size)
            ratio("Cornell box K = %d plain / MIS" % K, fig[False], fig[True], size)
    from power_scenes import unequal_lights

    utris, umats = (np.array(a) for a in unequal_lights())
    for size in SIZES:
        for mis in (False, True):
            fig = {}
            for choice in ("uniform", "power"):
                fig[choice] = leg(dev, "unequal-lights room K = 1 %s, lights by %s" % ("MIS" if mis else "plain", choice),
                                  lambda s, m: IndirectRenderer(dev, utris, umats, s, s, max_bounces=16, light_samples=1, mis=mis, light_choice=choice,
                                                                stripe_rows=1, moments=m), size)
            ratio("unequal-lights room K = 1 %s uniform / power" % ("MIS" if mis else "plain"), fig["uniform"], fig["power"], size)
    stris, smats = scene.make_soup()
    smats["emissive"][18::64, :3] = 30.0          # every 64th soup material emits (tools/direct_rates.py's soup)
    lights = scene.emitters(stris, smats)
    for size in SIZES:
        fig = {}
        for choice in ("uniform", "power"):
            fig[choice] = leg(dev, "soup, %d triangles, %d lights, direct K = 4, lights by %s" % (len(stris), len(lights), choice),
                              lambda s, m: DirectRenderer(dev, stris, smats, s, s, light_samples=4, lights=lights, light_choice=choice, stripe_rows=1,
                                                          moments=m), size)
        ratio("soup direct K = 4 uniform / power", fig["uniform"], fig["power"], size)
    for size in SIZES:
        accumulate_alone(dev, size)
finally:
    adl.DeviceUtils.deallocate(dev)
