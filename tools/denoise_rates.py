#!/usr/bin/env python3
"""Informational: what pt_denoise costs, by device events (pt_event_elapsed_ns), on the Cornell box at 1024^2 after `frames` frames of
IndirectRenderer(moments=True), all four guides.  Every figure is the median of `reps` timed calls after one warm-up, with the spread
(max - min) / median.
  (c) the call: ms per pt_denoise of 0 .. 5 levels under PT_OPT_DENOISE_TILE 1 (global gathers), 2 (LDS halo tile at steps 1 and 2) and 0
      (what ships);
      a level's time is the difference of the medians of two level counts, prepare's is the call of 0 levels;
  (m) the yardstick: a pt_buffer_copy of 40 bytes per pixel -- the 80 bytes of traffic a level must at least move (four float4 planes
      read, one written) -- in the same process, before and after the calls: its two medians bound the box's own drift;
  (s) for scale: the `frames` rendered frames the call filters and pt_render_features + moments for them, host-timed around a wait.
usage: python tools/denoise_rates.py [reps] [frames]"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.denoise import DEFAULTS  # noqa: E402
from oclpathtracer_amd.features import FEATURES  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 16
W = H = 1024
LEVELS = 5


def emit(**rec):
    print(json.dumps(rec), flush=True)


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, (ts[-1] - ts[0]) / med


def timed(dev, ev, call):
    ts = []
    for k in range(reps + 1):
        call()
        dev.waitForCompletion()
        if k:
            ts.append(ev.getExecutionTimeNanoseconds() * 1e-6)
    return stats(ts)


assert adl.init()
dev = adl.DeviceUtils.allocate()
lib = shim.load()
tris, mats = scene.load_model()
r = IndirectRenderer(dev, tris, mats, W, H, moments=True, stripe_rows=1)
ev = adl.SyncObject(dev)
copy_src = adl.Buffer(dev, 40 * W * H, np.uint8)
copy_dst = adl.Buffer(dev, 40 * W * H, np.uint8)
try:
    r.render(frames, 0)            # warm: the scene's tables
    dev.waitForCompletion()
    t0 = time.perf_counter()
    r.render(frames, 0)
    dev.waitForCompletion()
    render_ms = (time.perf_counter() - t0) * 1e3
    d, f = r.denoiser()
    t0 = time.perf_counter()
    f.render(frames, 0)
    dev.waitForCompletion()
    feature_ms = (time.perf_counter() - t0) * 1e3
    emit(leg="s", what="IndirectRenderer.render, %d frames of %d x %d (host-timed around a wait)" % (frames, W, H), ms=round(render_ms, 3))
    emit(leg="s", what="FeatureRenderer.render, four features and their moments, the same frames", ms=round(feature_ms, 3))

    copy = lambda: shim.check(lib.pt_buffer_copy(copy_dst._h, copy_src._h, 40 * W * H, 0, 0, ev._h))
    m0, ms0 = timed(dev, ev, copy)
    emit(leg="m", what="pt_buffer_copy of 40 bytes per pixel (first run)", median_ms=round(m0, 4), spread=round(ms0, 4),
         GBps_moved=round(80 * W * H / m0 * 1e-6, 1))

    guides = [f.mom[name]._h for name in FEATURES]
    med = {}
    for gather in (1, 2, 0):
        dev.setOption(shim.PT_OPT_DENOISE_TILE, gather)
        for levels in range(LEVELS + 1):
            p = shim.DenoiseParams()
            p.width, p.height = W, H
            for k, v in DEFAULTS.items():
                setattr(p, k, v)
            p.levels = levels
            call = lambda: shim.check(lib.pt_denoise(dev._h, r.mom._h, *guides, d.scratch._h, d.out._h, ctypes.byref(p), ev._h))
            med[gather, levels], s = timed(dev, ev, call)
            emit(leg="c", gather=gather, levels=levels, median_ms=round(med[gather, levels], 4), spread=round(s, 4))
    dev.setOption(shim.PT_OPT_DENOISE_TILE, 0)
    m1, ms1 = timed(dev, ev, copy)
    emit(leg="m", what="pt_buffer_copy of 40 bytes per pixel (second run)", median_ms=round(m1, 4), spread=round(ms1, 4),
         GBps_moved=round(80 * W * H / m1 * 1e-6, 1))
    m = 0.5 * (m0 + m1)
    emit(copy_run_to_run=round(abs(m1 - m0) / m, 4))
    for gather in (1, 2, 0):
        emit(leg="prepare", gather=gather, ms=round(med[gather, 0], 4))
        for i in range(LEVELS):
            ms = med[gather, i + 1] - med[gather, i]
            emit(leg="level", gather=gather, step=1 << i, ms=round(ms, 4), over_copy=round(ms / m, 3))
        emit(leg="call", gather=gather, levels=LEVELS, ms=round(med[gather, LEVELS], 4), over_render=round(med[gather, LEVELS] / render_ms, 5),
             over_features=round(med[gather, LEVELS] / feature_ms, 5))
    d.release()
    f.release()
finally:
    for b in (copy_src, copy_dst, ev):
        b.release()
    r.release()
    adl.DeviceUtils.deallocate(dev)
