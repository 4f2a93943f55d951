#!/usr/bin/env python3
"""Informational: samples/s of indirect illumination on the device (pt_render_indirect) on the Cornell box, 1024^2, 16 frames,
B = 16 bounces -- K = 0 (no light list: the renderer's estimator through the lock-step brute-force kernel), K = 1 and K = 4 light
samples per vertex, each of the latter two also with multiple importance sampling (pt_render_indirect_mis, the "mis" rows), and
K = 1 of both estimators through the LBVH kernels (PT_OPT_ACCEL 2), which the 36-triangle scene does not take by itself -- beside
pt_render_frames at the same size and depth in the same process.  Each leg is warmed up once at its
own shape (scene preparation, code objects), then run ONCE: a host clock around the enqueue and the device synchronise that ends
it.  The sample workspace holds all 16 frames, so an indirect render is one launch and one fold.
The K = 0 figure against the renderer's is what the brute-force kernel's missing lane regeneration costs.
With --lights power the legs are those of light choice by power instead: K = 1 and K = 4, plain and MIS, each with the uniform choice
and with the choice by power (pt_render_indirect_power) -- the same warm-up and single timed run per leg.
With --roulette the legs are those of Russian roulette (pt_render_indirect_rr, R = 3 and cap = 0.95 unless --roulette-setting R,cap says
otherwise): on the Cornell box and on the 10^6-triangle soup with every 64th material emissive, K = 0 (no lights), 1 and 4, plain and
MIS, three renders each in the same process -- the parent entry point, pt_render_indirect_rr with first_bounce = B (no roulette is
played: on the Cornell box the parent's image by the REFILLING brute-force kernel, so its rate against the parent's is what the missing
lane regeneration costs) and pt_render_indirect_rr with the roulette.  Each also renders once with moments=True, and the leg reports
efficiency = 1 / (variance per sample x time per sample) without and with roulette.
usage: python tools/indirect_rates.py [--lights power | --roulette [--roulette-setting R,cap]] [out.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oclpathtracer_amd import adl, scene, shim  # noqa: E402
from oclpathtracer_amd.indirect import IndirectRenderer  # noqa: E402
from oclpathtracer_amd.render import Renderer  # noqa: E402

power = "--lights" in sys.argv
if power:
    at = sys.argv.index("--lights")
    assert sys.argv[at + 1: at + 2] == ["power"], "--lights takes power"
    del sys.argv[at: at + 2]
roulette = "--roulette" in sys.argv
if roulette:
    sys.argv.remove("--roulette")
RR_SETTING = (3, 0.95)
if "--roulette-setting" in sys.argv:
    at = sys.argv.index("--roulette-setting")
    RR_SETTING = (int(sys.argv[at + 1].split(",")[0]), float(sys.argv[at + 1].split(",")[1]))
    del sys.argv[at: at + 2]
out_path = sys.argv[1] if len(sys.argv) > 1 else None
W = H = 1024
FRAMES, B = 16, 16


def emit(line):
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def once(dev, render):
    render()                       # warm-up, same shape
    dev.waitForCompletion()
    t0 = time.perf_counter()
    render()
    dev.waitForCompletion()
    return time.perf_counter() - t0


def report(name, t):
    n = W * H * FRAMES
    emit("%-44s %9.3f ms  %9.1f Msamples/s" % (name, t * 1e3, n / t / 1e6))
    return n / t


def roulette_legs(dev):
    from oclpathtracer_amd.indirect import Roulette

    soup_t, soup_m = scene.make_soup()
    soup_m["emissive"][18::64, :3] = 30.0          # every 64th soup material emits (tools/direct_rates.py's soup)
    emit("%s; %d x %d, %d frames, B = %d, roulette R = %d cap = %g; one warm-up and one timed run per render; variance per sample from the "
         "renderer's moments over the same %d frames" % ((dev.getDeviceName(), W, H, FRAMES, B) + RR_SETTING + (FRAMES,)))
    for scene_name, (t, m) in (("Cornell box", scene.load_model()), ("soup, %d triangles" % len(soup_t), (soup_t, soup_m))):
        for K, mis in ((0, False), (1, False), (1, True), (4, False), (4, True)):
            lights = np.zeros(0, np.int32) if K == 0 else None
            fig = {}
            for what, rr in (("parent entry point", None), ("rr, first_bounce = B (no roulette)", Roulette(B, 1.0)), ("rr, roulette", Roulette(*RR_SETTING))):
                kw = dict(light_samples=max(K, 1), lights=lights, max_bounces=B, stripe_rows=1, chunk_frames=FRAMES, mis=mis, roulette=rr)
                ir = IndirectRenderer(dev, t, m, W, H, **kw)
                im = IndirectRenderer(dev, t, m, W, H, moments=True, **kw)
                try:
                    sec = once(dev, lambda: ir.render(FRAMES, 0))
                    im.render(FRAMES, 0)
                    var = im.noise().variance_per_sample
                finally:
                    ir.release()
                    im.release()
                name = "%s K = %d%s: %s" % (scene_name, K, " MIS" if mis else "", what)
                rate = W * H * FRAMES / sec
                fig[what] = (rate, var)
                emit("%-72s %9.3f ms  %9.1f Msamples/s  variance per sample %-11.5g efficiency %.5g" % (name, sec * 1e3, rate / 1e6, var, rate / var))
            parent = fig["parent entry point"]
            for what in list(fig)[1:]:
                emit("%-72s %9.3f of the parent's rate, %.3f of its variance per sample, %.3f of its efficiency"
                     % ("", fig[what][0] / parent[0], fig[what][1] / parent[1], (fig[what][0] / fig[what][1]) / (parent[0] / parent[1])))


assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    if roulette:
        roulette_legs(dev)
        sys.exit(0)
    tris, mats = scene.load_model()
    emit("%s; Cornell box, %d x %d, %d frames, B = %d; one warm-up and one timed run per leg" % (dev.getDeviceName(), W, H, FRAMES, B))
    r = Renderer(dev, tris, mats, W, H, stripe_rows=1)
    try:
        base = report("pt_render_frames", once(dev, lambda: r.render(FRAMES, frame_begin=0, max_bounces=B)))
    finally:
        r.release()
    if power:
        for K in (1, 4):
            for mis in (False, True):
                uniform = None
                for choice in ("uniform", "power"):
                    ir = IndirectRenderer(dev, tris, mats, W, H, light_samples=K, max_bounces=B, stripe_rows=1, chunk_frames=FRAMES, mis=mis, light_choice=choice)
                    try:
                        entry = "pt_render_indirect_power mis = %d" % mis if choice == "power" else "pt_render_indirect_mis" if mis else "pt_render_indirect"
                        rate = report("%s K = %d" % (entry, K), once(dev, lambda: ir.render(FRAMES, 0)))
                        if choice == "power":
                            emit("%-44s %9.3f of the uniform choice's rate at the same K and estimator" % ("", rate / uniform))
                        uniform = rate
                    finally:
                        ir.release()
        sys.exit(0)
    plain = {}
    for name, K, lights, mis, accel in (("pt_render_indirect K = 0 (no lights)", 1, np.zeros(0, np.int32), False, 0),
                                        ("pt_render_indirect K = 1", 1, None, False, 0), ("pt_render_indirect_mis K = 1", 1, None, True, 0),
                                        ("pt_render_indirect K = 4", 4, None, False, 0), ("pt_render_indirect_mis K = 4", 4, None, True, 0),
                                        ("pt_render_indirect K = 1, LBVH", 1, None, False, 2), ("pt_render_indirect_mis K = 1, LBVH", 1, None, True, 2)):
        dev.setOption(shim.PT_OPT_ACCEL, accel)
        ir = IndirectRenderer(dev, tris, mats, W, H, light_samples=K, lights=lights, max_bounces=B, stripe_rows=1, chunk_frames=FRAMES, mis=mis)
        try:
            rate = report(name, once(dev, lambda: ir.render(FRAMES, 0)))
            emit("%-44s %9.3f of pt_render_frames' rate" % ("", rate / base))
            if mis:
                emit("%-44s %9.3f of the plain estimator's rate at the same K and search" % ("", rate / plain[K, accel]))
            elif lights is None:
                plain[K, accel] = rate
        finally:
            ir.release()
            dev.setOption(shim.PT_OPT_ACCEL, 0)
finally:
    adl.DeviceUtils.deallocate(dev)
