#!/usr/bin/env python3
"""Informational: what adaptive sampling (IndirectRenderer.render_adaptive) buys and what its list map costs, ON THE DEVICE.  One
process, one device, the Cornell box, MIS + lights by power + roulette (3, 0.95), B = 16, K = 1, moments kept.

Equal noise, twice.  First the target is the image's ``noise().relative_error`` after FRAMES uniform frames: the uniform leg is
``render_until`` to that target (one host wait per check), the adaptive leg ``render_adaptive`` with the largest per-pixel tolerance of
a bisection that reaches the same image-wide figure (untimed; printed), with passes of one workspace and of 64 frames.  Then the other
way round: the figure ``render_adaptive`` reaches with the target as its per-pixel tolerance, and the frames ``render_until`` needs for
it (at most 16 x FRAMES).  Both legs start at frame 0, are timed by a host clock around the calls and the synchronise that ends them,
and alternate REPS times after one warm-up pair; wall time and samples are reported with the spread (min .. max).

The list map alone: ``render_adaptive`` with tolerance 0 and floor 0, where every pixel of non-zero variance stays listed until
max_samples, against ``render`` with moments for the same frames.  Then the calls of one such pass by device events, each list call
beside its parent: pt_adaptive_select, pt_render_indirect_pixels against pt_render_indirect_rr, pt_sample_moments_pixels against
pt_sample_moments.
No figure is gated.  usage: python tools/adaptive_rates.py [rates.txt] [--size 1024] [--frames 256] [--reps 5]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette  # noqa: E402

args = sys.argv[1:]


def option(name, default):
    if name in args:
        at = args.index(name)
        value = args[at + 1]
        del args[at: at + 2]
        return value
    return default


SIZE = int(option("--size", 1024))
FRAMES = int(option("--frames", 256))
REPS = int(option("--reps", 5))
MIN_SAMPLES, MAX_SAMPLES = 16, 16 * FRAMES
out_path = (args + [None])[0]


def emit(line):
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def timed(dev, run):
    dev.waitForCompletion()
    t0 = time.perf_counter()
    result = run()
    dev.waitForCompletion()
    return time.perf_counter() - t0, result


def spread(values, scale=1.0, fmt="%.1f"):
    v = np.asarray(values, np.float64) * scale
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (float(np.median(v)), float(v.min()), float(v.max()))


assert adl.init()
dev = adl.DeviceUtils.allocate()
tris, mats = scene.load_model()
r = IndirectRenderer(dev, tris, mats, SIZE, SIZE, max_bounces=16, light_samples=1, mis=True, light_choice="power", roulette=Roulette(3, 0.95),
                     stripe_rows=1, moments=True)
try:
    npix, step = SIZE * SIZE, r.chunk_frames
    emit("%s; Cornell box %d^2, MIS, lights by power, roulette (3, 0.95), B = 16, K = 1; workspace of %d frames; medians of %d alternating runs "
         "after one warm-up pair, (min .. max)" % (dev.getDeviceName(), SIZE, step, REPS))

    def uniform(target, max_frames=FRAMES):
        r.render(step, 0)
        return r.render_until(target, max_frames) * npix

    def adaptive(tolerance, fpp=None):
        r.render(MIN_SAMPLES, 0)
        return r.render_adaptive(tolerance, min_samples=MIN_SAMPLES, max_samples=MAX_SAMPLES, frames_per_pass=fpp).samples + MIN_SAMPLES * npix

    def compare(what, target, tolerance, fpp, max_frames):
        """both legs to the image-wide figure ``target``, alternating"""
        tu, ta, su, sa, eu, ea = [], [], [], [], [], []
        for rep in range(REPS + 1):
            a, n_u = timed(dev, lambda: uniform(target, max_frames))
            e_u = r.noise().relative_error
            b, n_a = timed(dev, lambda: adaptive(tolerance, fpp))
            e_a, counts = r.noise().relative_error, r.sample_counts()
            if rep:
                tu.append(a), ta.append(b), su.append(n_u), sa.append(n_a), eu.append(e_u), ea.append(e_a)
        emit("%s, render_until:    %s ms, %s Msamples (%d frames), reaches %.6g" % (what, spread(tu, 1e3), spread(su, 1e-6), su[-1] // npix, eu[-1]))
        emit("%s, render_adaptive: %s ms, %s Msamples, reaches %.6g; tolerance %.6g, %d frames per pass; samples per pixel min %d median %d max %d; "
             "%.1f %% of the pixels stop at min_samples" % (what, spread(ta, 1e3), spread(sa, 1e-6), ea[-1], tolerance, fpp or step, int(counts.min()),
                                                            int(np.median(counts)), int(counts.max()), 100.0 * float((counts == MIN_SAMPLES).mean())))
        emit("%s, adaptive / uniform: time %.3f, samples %.3f" % (what, float(np.median(ta)) / float(np.median(tu)), float(np.median(sa)) / float(np.median(su))))

    # 1. the figure render_until reaches at FRAMES frames.  The image-wide figure is not monotone in the frames (a few pixels' rare, very
    # bright samples carry it), so render_until may pass it early; the adaptive tolerance is the largest of a bisection that reaches it
    uniform(0.0)
    target = r.noise().relative_error
    r.render(MIN_SAMPLES, 0)
    emit("target: relative_error %.6g after %d uniform frames (after %d: %.6g)" % (target, FRAMES, MIN_SAMPLES, r.noise().relative_error))
    lo, hi = target, 16.0 * target
    for _ in range(7):
        mid = (lo * hi) ** 0.5
        adaptive(mid)
        if r.noise().relative_error <= target:
            lo = mid
        else:
            hi = mid
    for fpp in (None, 64):
        compare("target of %d frames" % FRAMES, target, lo, fpp, FRAMES)
    # 2. the other way round: the figure the adaptive render reaches with the per-pixel tolerance `target`, and the uniform frames that need
    adaptive(target, 64)
    reached = r.noise().relative_error
    compare("adaptive's figure", reached, target, 64, 16 * FRAMES)

    k = 8                                      # the list map alone: k passes with (nearly) every pixel listed
    frames = MIN_SAMPLES + k * step

    def all_listed():
        r.render(MIN_SAMPLES, 0)
        return r.render_adaptive(0.0, min_samples=MIN_SAMPLES, max_samples=frames - step + 1, floor=0.0)

    tl, tr, listed = [], [], []
    for rep in range(REPS + 1):
        a, res = timed(dev, all_listed)
        b, _ = timed(dev, lambda: r.render(frames, 0))
        if rep:
            tl.append(a), tr.append(b), listed.append(res.samples + MIN_SAMPLES * npix)
    emit("list map alone: %d frames; render with moments %s ms; %d uniform frames + %d passes at tolerance 0 %s ms (%.4f of the samples: pixels "
         "of zero variance are not listed); ratio of times %.3f" % (frames, spread(tr, 1e3), MIN_SAMPLES, len(res.passes), spread(tl, 1e3),
                                                                   float(np.median(listed)) / (frames * npix), float(np.median(tl)) / float(np.median(tr))))

    # the calls of one pass by device events, every pixel listed, one workspace of frames: each list call beside its parent
    import ctypes

    from oclpathtracer_amd import shim

    ev = adl.SyncObject(dev)
    try:
        r.render(MIN_SAMPLES, 0)
        rule = shim.AdaptiveRule(0.0, 0.0, MIN_SAMPLES, MAX_SAMPLES)
        h = lambda b: b._h if b is not None else None
        lights = h(r.lbuf) if len(r.lights) else None
        p = r.params(step, MIN_SAMPLES)

        def by_events(call):
            ns = []
            for rep in range(10):
                shim.check(call())
                ev.waitForCompletion()
                ns.append(ev.getExecutionTimeNanoseconds())
            return float(np.median(ns[1:])) * 1e-3

        t_select = by_events(lambda: r._lib.pt_adaptive_select(dev._h, r.mom._h, npix, ctypes.byref(rule), r.pixel_list._h, ev._h))
        head = np.zeros(1, np.uint32)
        r.pixel_list.read(head, head.nbytes)
        dev.waitForCompletion()
        listed = int(head[0])
        t_parent = by_events(lambda: r._lib.pt_render_indirect_rr(dev._h, r.tbuf._h, r.mbuf._h, lights, 1, r.counts._h, r.cdf._h, r.tri_q._h, r.samples._h,
                                                                  r.fb._h, ctypes.byref(p), ctypes.byref(r._rr), None, ev._h))
        q = r.params(step, 0)
        t_list = by_events(lambda: r._lib.pt_render_indirect_pixels(dev._h, r.tbuf._h, r.mbuf._h, lights, 1, r.counts._h, r.cdf._h, r.tri_q._h, r.samples._h,
                                                                    r.fb._h, r.pixel_list._h, listed, ctypes.byref(q), ctypes.byref(r._rr), None, ev._h))
        m_parent = by_events(lambda: r._lib.pt_sample_moments(dev._h, r.samples._h, r.mom._h, npix, step, 0, ev._h))
        m_list = by_events(lambda: r._lib.pt_sample_moments_pixels(dev._h, r.samples._h, r.mom._h, r.pixel_list._h, listed, step, ev._h))
        emit("one pass by events (medians of 9), %d of %d pixels listed, %d frames: pt_adaptive_select %.1f us; render + fold: pt_render_indirect_rr %.1f us, "
             "pt_render_indirect_pixels %.1f us (%.3f); moments: pt_sample_moments %.1f us, pt_sample_moments_pixels %.1f us"
             % (listed, npix, step, t_select, t_parent, t_list, t_list / t_parent, m_parent, m_list))
    finally:
        ev.release()
finally:
    r.release()
    adl.DeviceUtils.deallocate(dev)
