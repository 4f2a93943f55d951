#!/usr/bin/env python3
"""Informational: G rays/s of direct illumination on the device (pt_render_direct), beside ambient occlusion (pt_render_ao) on
the same box in the same run at the same K -- both do one closest search plus up to K any-hit searches per sample; direct
illumination adds a light gather and a BRDF value per shadow ray.  Every leg is warmed up once, then timed `reps` times by its own
device event pair (the direct render's pair spans its launch AND its fold); the median is recorded (one JSON line each).
  (a) Cornell box 1024^2, 1 frame, K = 16: pt_render_direct, then pt_render_ao at radius 1e20.
  (b) the 10^6-triangle soup (scene.make_soup) 1024^2, 1 frame, K = 4, one soup material in 64 made emissive here (make_soup has
      none): pt_render_direct with the soup's emitters and the box's light in the list, then pt_render_ao at radius 1.0.
Rays = the primary rays (npix x frames) + the shadow rays cast.  The device does not count the rays it casts: the count comes from
the CPU restatement of the estimator (tests/direct_oracle.c) -- over every sample of the box, over a fixed random subset of
`subset` samples of the soup, whose cast fraction is then an estimate (the line says which).
With --lights power the legs are those of light choice by power instead (pt_render_direct_power beside pt_render_direct, no ambient
occlusion, no ray count): (c) the Cornell box 1024^2, 16 frames in one launch and one fold, K = 1 and K = 4, each choice warmed up once
and run ONCE under a host clock; (d) the soup of (b), 1 frame, K = 4, both choices likewise, and pt_light_table for the soup's list timed
`reps` times by a device event pair (the median).
usage: python tools/direct_rates.py [--lights power] [reps] [out.jsonl] [subset]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import direct_oracle  # noqa: E402
from oclpathtracer_amd import adl, scene  # noqa: E402
from oclpathtracer_amd.ao import AORenderer  # noqa: E402
from oclpathtracer_amd.direct import DirectRenderer  # noqa: E402

power = "--lights" in sys.argv
if power:
    at = sys.argv.index("--lights")
    assert sys.argv[at + 1: at + 2] == ["power"], "--lights takes power"
    del sys.argv[at: at + 2]
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None
subset = int(sys.argv[3]) if len(sys.argv) > 3 else 192


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def timed(dev, render):
    ev = adl.SyncObject(dev)
    try:
        render(ev)
        dev.waitForCompletion()
        ts = []
        for _ in range(reps):
            render(ev)
            dev.waitForCompletion()
            ts.append(ev.getExecutionTimeNanoseconds() * 1e-9)
    finally:
        ev.release()
    return median(ts)


def cast_rays(tris, mats, lights, W, H, K, gids):
    """(primary hits, shadow rays cast) among the samples gids of frame 0, from the restatement's decisions"""
    hit, dec, _ = direct_oracle.decisions(tris, mats, W, H, gids, np.zeros(len(gids)), K, lights=lights)
    return int(hit.sum()), int((dec != direct_oracle.NONE).sum())


def leg(dev, name, tris, mats, lights, W, H, K, radius, gids):
    d = DirectRenderer(dev, tris, mats, W, H, light_samples=K, lights=lights, stripe_rows=1, chunk_frames=1)
    try:
        t = timed(dev, lambda ev: d.render(1, 0, sync=ev))
        a = AORenderer(dev, d.tbuf, W, H, rays_per_sample=K, radius=radius, num_triangles=len(tris), stripe_rows=1)
        try:
            ta = timed(dev, lambda ev: a.render(1, 0, sync=ev))
            ao_rays = W * H + K * int(a.read_counts()[..., 1].astype(np.int64).sum())
        finally:
            a.release()
    finally:
        d.release()
    hits, cast = cast_rays(tris, mats, lights, W, H, K, gids)
    exact = len(gids) == W * H
    rays = W * H + (cast if exact else int(round(cast * (W * H / len(gids)))))
    emit({"leg": name, "what": "pt_render_direct %d^2 x 1 frame" % W, "K": K, "lights": int(len(lights)), "reps": reps,
          "median_ms": round(t * 1e3, 3), "rays": rays, "rays_counted": "exact" if exact else "estimated from %d samples" % len(gids),
          "shadow_rays_per_light_sample": round(cast / max(1, K * hits), 4), "grays_per_s": round(rays / t / 1e9, 3)})
    emit({"leg": name, "what": "pt_render_ao %d^2 x 1 frame" % W, "K": K, "radius": radius, "reps": reps,
          "median_ms": round(ta * 1e3, 3), "rays": ao_rays, "grays_per_s": round(ao_rays / ta / 1e9, 3),
          "direct_over_ao_time": round(t / ta, 3), "direct_over_ao_rate": round((rays / t) / (ao_rays / ta), 3)})


def power_leg(dev, name, tris, mats, lights, W, H, K, frames):
    """pt_render_direct beside pt_render_direct_power: one warm-up and one run each under a host clock; the table build by events"""
    import time

    from oclpathtracer_amd import shim

    rate = {}
    for choice in ("uniform", "power"):
        d = DirectRenderer(dev, tris, mats, W, H, light_samples=K, lights=lights, stripe_rows=1, chunk_frames=frames, light_choice=choice)
        try:
            d.render(frames, 0)
            dev.waitForCompletion()
            t0 = time.perf_counter()
            d.render(frames, 0)
            dev.waitForCompletion()
            t = time.perf_counter() - t0
            rate[choice] = W * H * frames / t
            rec = {"leg": name, "what": "pt_render_direct%s %d^2 x %d frames" % ("_power" if choice == "power" else "", W, frames), "K": K,
                   "lights": int(len(lights)), "light_choice": choice, "runs": 1, "ms": round(t * 1e3, 3), "msamples_per_s": round(rate[choice] / 1e6, 2)}
            if choice == "power":
                rec["power_over_uniform_rate"] = round(rate["power"] / rate["uniform"], 3)
                tb = timed(dev, lambda ev: shim.check(d._lib.pt_light_table(dev._h, d.tbuf._h, d.num_triangles, d.mbuf._h, d.num_materials, d.lbuf._h,
                                                                            len(d.lights), d.cdf._h, d.tri_q._h, ev._h)))
                rec["table_build_median_ms"], rec["table_build_reps"] = round(tb * 1e3, 4), reps
            emit(rec)
        finally:
            d.release()


assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    W = H = 1024
    tris, mats = scene.load_model()
    if power:
        for K in (1, 4):
            power_leg(dev, "cornell", tris, mats, scene.emitters(tris, mats), W, H, K, 16)
        tris, mats = scene.make_soup()
        mats["emissive"][18::64, :3] = 30.0          # every 64th soup material emits, as in (b)
        power_leg(dev, "soup", tris, mats, scene.emitters(tris, mats), W, H, 4, 1)
        sys.exit(0)
    leg(dev, "cornell", tris, mats, scene.emitters(tris, mats), W, H, 16, 1e20, np.arange(W * H))
    tris, mats = scene.make_soup()
    mats["emissive"][18::64, :3] = 30.0          # every 64th soup material emits
    lights = scene.emitters(tris, mats)
    gids = np.sort(np.random.default_rng(7).choice(W * H, subset, replace=False))
    leg(dev, "soup", tris, mats, lights, W, H, 4, 1.0, gids)
finally:
    adl.DeviceUtils.deallocate(dev)
