#!/usr/bin/env python3
"""Informational: what pt_reproject costs, by device events (pt_event_elapsed_ns), on the Cornell box at 1024^2: a history of `frames`
frames of IndirectRenderer(moments=True) under the reference camera, the eye (and centre) moved by 0.1 along x, one feature frame under
the new camera.  Every figure is the median of `reps` timed calls after one warm-up, with the spread (max - min) / median.
  (c) the call: ms per pt_reproject under PT_OPT_REPROJECT_FORM 1 (one kernel over the records), 2 (a prepare pass first) and 0 (what
      ships), with and without the normal test and the info map;
  (m) the yardstick: a pt_buffer_copy of half the bytes a call must at least move -- counted here from the record sizes: five moment
      records read, one record and one float4 written, per pixel -- in the same process, before and after the calls: its two medians
      bound the box's own drift;
  (s) for scale: one lit frame, and one feature frame with its moments, at that size, host-timed around a wait.
usage: python tools/reproject_rates.py [reps] [frames]"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.camera import Camera  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 16
W = H = 1024
RECORD, INFO = ctypes.sizeof(shim.PixelMoments), 16
READ, WRITTEN = 5 * RECORD, RECORD + INFO     # prev colour, normal, depth and cur normal, depth; out colour and info
MOVED = READ + WRITTEN
COPY = MOVED // 2                             # a copy of COPY bytes per pixel reads and writes that: MOVED bytes per pixel moved


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
copy_src = adl.Buffer(dev, COPY * W * H, np.uint8)
copy_dst = adl.Buffer(dev, COPY * W * H, np.uint8)
out = adl.Buffer(dev, RECORD * W * H, np.uint8)
acc = None
try:
    emit(bytes_per_pixel=dict(read=READ, written=WRITTEN, moved=MOVED, copied_by_the_yardstick=COPY))
    acc = r.temporal()
    acc.render(frames - 1)         # (warm: the scene's tables); the last frame of the history is the one timed for scale
    dev.waitForCompletion()
    t0 = time.perf_counter()
    r.render(1)
    dev.waitForCompletion()
    lit_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    acc.features.render(1)
    dev.waitForCompletion()
    feature_ms = (time.perf_counter() - t0) * 1e3
    emit(leg="s", what="IndirectRenderer.render, one frame of %d x %d and its moments (host-timed around a wait)" % (W, H), ms=round(lit_ms, 3))
    emit(leg="s", what="FeatureRenderer.render, one frame of four features and their moments", ms=round(feature_ms, 3))

    moved = Camera((0.1, 2.75, 4.0), (0.1, 2.75, 3.0))
    prev, cur = acc.features, acc._previous
    cur._set_camera(moved)
    cur.render(1, r.frames_done, restart=True)
    dev.waitForCompletion()
    cs = moved.to_struct()

    copy = lambda: shim.check(lib.pt_buffer_copy(copy_dst._h, copy_src._h, COPY * W * H, 0, 0, ev._h))
    m0, ms0 = timed(dev, ev, copy)
    emit(leg="m", what="pt_buffer_copy of %d bytes per pixel (first run)" % COPY, median_ms=round(m0, 4), spread=round(ms0, 4),
         GBps_moved=round(MOVED * W * H / m0 * 1e-6, 1))

    p = acc.reprojector.params
    med = {}
    for normals, info in ((True, True), (False, True), (True, False)):
        for form in (1, 2, 0):
            dev.setOption(shim.PT_OPT_REPROJECT_FORM, form)
            h = lambda f, name: f.mom[name]._h
            call = lambda: shim.check(lib.pt_reproject(dev._h, r.mom._h, h(prev, "normal") if normals else None, h(prev, "depth"),
                                                       h(cur, "normal") if normals else None, h(cur, "depth"), acc.reprojector.scratch._h, out._h,
                                                       acc.info_buf._h if info else None, ctypes.byref(p), None, ctypes.byref(cs), ev._h))
            med[form, normals, info], s = timed(dev, ev, call)
            emit(leg="c", form=form, normals=normals, info=info, median_ms=round(med[form, normals, info], 4), spread=round(s, 4))
    dev.setOption(shim.PT_OPT_REPROJECT_FORM, 0)
    took = np.zeros((W * H, 4), np.float32)
    acc.info_buf.read(took, W * H)
    dev.waitForCompletion()
    emit(leg="c", what="pixels that took history", share=round(float((took[:, 3] > 0).mean()), 4), mean_length=round(float(took[took[:, 3] > 0, 3].mean()), 3))
    m1, ms1 = timed(dev, ev, copy)
    emit(leg="m", what="pt_buffer_copy of %d bytes per pixel (second run)" % COPY, median_ms=round(m1, 4), spread=round(ms1, 4),
         GBps_moved=round(MOVED * W * H / m1 * 1e-6, 1))
    m = 0.5 * (m0 + m1)
    emit(copy_run_to_run=round(abs(m1 - m0) / m, 4))
    for form in (1, 2, 0):
        ms = med[form, True, True]
        emit(leg="call", form=form, ms=round(ms, 4), over_copy=round(ms / m, 3), over_lit_frame=round(ms / lit_ms, 5), over_feature_frame=round(ms / feature_ms, 5))
finally:
    if acc is not None:
        acc.release()
    for b in (copy_src, copy_dst, out, ev):
        b.release()
    r.release()
    adl.DeviceUtils.deallocate(dev)
