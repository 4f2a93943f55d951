#!/usr/bin/env python3
"""Informational: Msamples/s of a configs[2]-sized render (1024 x 1024, 256 samples per pixel, depth 16) of the Cornell box
from the reference's viewpoint and three moved ones (the camera is a runtime value of every trace kernel; the pass-1
filters' anchor moves with the eye).  One JSON line per camera.
usage: python tools/camera_rates.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oclpathtracer_amd import adl, scene  # noqa: E402
from oclpathtracer_amd.camera import Camera  # noqa: E402
from oclpathtracer_amd.render import Renderer  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W = H = 1024
SPP = 256
cams = {
    "reference": None,
    "yawed30": Camera((0.0, 2.75, 4.0), (-0.5, 2.75, 4.0 - 0.8660254)),
    "inside_up": Camera((0.3, 1.5, -2.5), (0.0, 5.4, -2.8), up=(0.0, 0.0, -1.0)),
    "far_fov20": Camera((0.0, 2.75, 54.0), (0.0, 2.75, -2.8), fov_y_deg=20.0),
}
tris, mats = scene.load_model()
assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    r = Renderer(dev, tris, mats, W, H)
    for name, cam in cams.items():
        r.set_camera(cam)
        r.render(SPP, frame_begin=0)          # warm: tables, masks
        dev.waitForCompletion()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r.render(SPP, frame_begin=0)
            dev.waitForCompletion()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        med = ts[len(ts) // 2]
        print(json.dumps({"camera": name, "W": W, "H": H, "spp": SPP, "depth": 16, "reps": reps, "median_ms": round(med * 1e3, 3),
                          "min_ms": round(ts[0] * 1e3, 3), "msamples_per_s": round(W * H * SPP / med / 1e6, 1)}), flush=True)
    r.release()
finally:
    adl.DeviceUtils.deallocate(dev)
