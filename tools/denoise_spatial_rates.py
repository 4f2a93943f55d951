#!/usr/bin/env python3
"""Informational: what pt_denoise_spatial costs beside pt_denoise, by device events (pt_event_elapsed_ns), on the Cornell box at 1024^2,
IndirectRenderer(moments=True), all four guides, five levels (and none: prepare, or prepare and the pool, alone).  Every figure is the
median of `reps` timed calls after one warm-up, with the spread (max - min) / median.  Three sets of records:
  long   16 frames: no pixel is short, every workgroup of the pool pass leaves at its vote;
  one    1 frame: every pixel is short, under PT_OPT_DENOISE_SPATIAL_FORM 1 (global gathers), 2 (LDS tile) and 0 (what ships);
  moved  a TemporalAccumulator after 16 frames, a move of the eye by 0.1 and one new frame: the pixels without history are short.
On a library without pt_denoise_spatial (the parent commit's) only pt_denoise is timed; `--baseline FILE` takes such a run's output
and states every figure as a ratio to that run's pt_denoise on the same records.
usage: python tools/denoise_spatial_rates.py [reps] [--baseline FILE]"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.camera import Camera  # noqa: E402
from oclpathtracer_amd.denoise import DEFAULTS  # noqa: E402
from oclpathtracer_amd.features import FEATURES  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer  # noqa: E402

args = sys.argv[1:]
baseline = {}
if "--baseline" in args:
    i = args.index("--baseline")
    for line in open(args[i + 1]):
        rec = json.loads(line) if line.startswith("{") else {}
        if rec.get("call") == "pt_denoise":
            baseline[rec["records"], rec["levels"]] = rec["median_ms"]
    del args[i:i + 2]
reps = int(args[0]) if args else 9
W = H = 1024
LONG = 16
SPATIAL = "pt_denoise_spatial" in shim.SIGNATURES


def emit(**rec):
    print(json.dumps(rec), flush=True)


def timed(dev, ev, call):
    ts = []
    for k in range(reps + 1):
        call()
        dev.waitForCompletion()
        if k:
            ts.append(ev.getExecutionTimeNanoseconds() * 1e-6)
    ts.sort()
    return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]


assert adl.init()
dev = adl.DeviceUtils.allocate()
lib = shim.load()
tris, mats = scene.load_model()
ev = adl.SyncObject(dev)
scratch = adl.Buffer(dev, lib.pt_denoise_scratch_bytes(W, H), np.uint8)
out = adl.Buffer(dev, W * H, adl.float4)
med = {}


def measure(records, colour, features):
    """every call on one set of records"""
    rec = np.zeros(W * H, np.dtype([("sum", np.float64, 3), ("sum2", np.float64, 3), ("n", np.uint32), ("rejected", np.uint32)]))
    colour.read(rec.view(np.uint8), rec.nbytes)
    dev.waitForCompletion()
    short = int((rec["n"] == 1).sum())
    tiles = (rec["n"] == 1).reshape(H // 8, 8, W // 32, 32).any(axis=(1, 3))
    emit(records=records, pixels=W * H, short_pixels=short, tiles=int(tiles.size), tiles_with_a_short_pixel=int(tiles.sum()))
    guides = [features.mom[name]._h for name in FEATURES]
    for levels in (5, 0):
        p = shim.DenoiseParams()
        p.width, p.height = W, H
        for k, v in DEFAULTS.items():
            setattr(p, k, v)
        p.levels = levels
        m, s = timed(dev, ev, lambda: shim.check(lib.pt_denoise(dev._h, colour._h, *guides, scratch._h, out._h, ctypes.byref(p), ev._h)))
        med[records, "pt_denoise", 0, levels] = m
        rec = dict(records=records, call="pt_denoise", levels=levels, median_ms=round(m, 4), spread=round(s, 4))
        if (records, levels) in baseline:
            rec["over_baseline"] = round(m / baseline[records, levels], 4)
        emit(**rec)
        if not SPATIAL:
            continue
        sp = shim.DenoiseSpatialParams()
        sp.below = 2
        for form in ((0,) if records == "long" else (1, 2, 0)):
            dev.setOption(shim.PT_OPT_DENOISE_SPATIAL_FORM, form)
            m, s = timed(dev, ev, lambda: shim.check(lib.pt_denoise_spatial(dev._h, colour._h, *guides, scratch._h, out._h, ctypes.byref(p),
                                                                            ctypes.byref(sp), ev._h)))
            med[records, "pt_denoise_spatial", form, levels] = m
            rec = dict(records=records, call="pt_denoise_spatial", below=2, form=form, levels=levels, median_ms=round(m, 4), spread=round(s, 4),
                       over_pt_denoise_here=round(m / med[records, "pt_denoise", 0, levels], 4))
            if (records, levels) in baseline:
                rec["over_baseline"] = round(m / baseline[records, levels], 4)
            emit(**rec)
        dev.setOption(shim.PT_OPT_DENOISE_SPATIAL_FORM, 0)


try:
    for records, frames in (("long", LONG), ("one", 1)):
        r = IndirectRenderer(dev, tris, mats, W, H, moments=True, stripe_rows=1)
        d = f = None
        try:
            r.render(frames, 0)
            d, f = r.denoiser()
            measure(records, r.mom, f)
        finally:
            for o in (d, f):
                if o is not None:
                    o.release()
            r.release()
    r = IndirectRenderer(dev, tris, mats, W, H, moments=True, stripe_rows=1)
    acc = None
    try:
        acc = r.temporal()
        acc.render(LONG)
        eye, centre = Camera.reference().eye, Camera.reference().center
        acc.move(Camera((eye[0] + 0.1, eye[1], eye[2]), (centre[0] + 0.1, centre[1], centre[2])))
        acc.render(1)
        measure("moved", r.mom, acc.features)
    finally:
        if acc is not None:
            acc.release()
        r.release()
    if SPATIAL:
        for records in ("long", "one", "moved"):
            for form in ((0,) if records == "long" else (1, 2, 0)):
                pool = med[records, "pt_denoise_spatial", form, 0] - med[records, "pt_denoise", 0, 0]
                emit(leg="pool pass alone (the calls of 0 levels, spatial minus plain)", records=records, form=form, ms=round(pool, 4),
                     over_five_levels=round(pool / (med[records, "pt_denoise", 0, 5] - med[records, "pt_denoise", 0, 0]), 4))
finally:
    for b in (scratch, out, ev):
        b.release()
    adl.DeviceUtils.deallocate(dev)
