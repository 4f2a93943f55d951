"""The inputs of tests/test_gpu_roulette.py and what the restatement (tests/roulette_oracle.c) says of them: one table, so that
tests/test_roulette_cpu.py proves on exactly the scenes and sizes the device renders that every edge of the roulette is reached.
TEST INFRASTRUCTURE.

An estimator is (mis, power); a roulette setting (R, cap); a scene a name of scenes.edge_scene."""
from __future__ import annotations

import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import direct_oracle as do
import roulette_oracle as ro
from conftest import ROOT
from scenes import edge_scene

ESTIMATORS = ((False, False), (True, False), (False, True), (True, True))   # (mis, power)
EST_IDS = ["plain", "mis", "power", "mis_power"]
SETTINGS = tuple((R, cap) for R in (1, 3) for cap in (1.0, 0.95, 0.25))      # the parity matrix
W, H, FRAMES, B = 24, 16, 3, 16                                            # the Cornell box of the parity matrix, K = 1 and 2
KS = (1, 2)
GLOSSY = ("finite:5", 2, 6)                                                # one glossy finite room: (scene, K, B)
LBVH = ("nested:15", 2, 6)                                                 # 540 triangles: PT_OPT_ACCEL 0 takes the LBVH
TILED = ("nested:10", 2, 6)                                                # 360 triangles: the LDS_TABLE = 2 instantiations
BIG_SETTINGS = ((1, 0.25), (3, 0.95))                                      # the settings of the three scenes above

# the roulette's edges: name -> (scene, W, H, frames, K, B, R, cap, mis).  tests/test_roulette_cpu.py proves each is reached
EDGES = {
    "q_at_least_one": ("finite:5", 24, 16, 3, 1, 6, 1, 1.0, True),        # a glossy mask above 1: the path goes on, mask unchanged
    "capped": ("cornell", 24, 16, 3, 1, 6, 1, 0.25, True),                # s > cap, q = cap < 1
    "nan_mask": ("glossy:0", 24, 16, 3, 1, 6, 1, 0.95, True),             # a NaN mask: the path must end
    "nonpositive": ("cornell", 24, 16, 3, 1, 6, 1, 0.95, False),          # s <= 0: the path must end
    "first_eligible": ("cornell", 24, 16, 3, 1, 6, 3, 0.25, False),       # ended by the roulette at vertex R - 1
    "survivor": ("cornell", 24, 16, 3, 1, 4, 1, 0.95, True),              # survives every roulette to vertex B - 1
}


def rr_run() -> int:
    """PT_RR_RUN of csrc/pt_constants.h: the items a wave of the brute-force roulette kernel owns"""
    text = open(os.path.join(ROOT, "oclpathtracer_amd", "csrc", "pt_constants.h")).read()
    return int(re.search(r"^#define PT_RR_RUN (\d+)\s*$", text, re.M).group(1))


def refill_counts():
    """item counts per launch about a wave and about a run"""
    run = rr_run()
    return [1, 63, 64, 65, run - 1, run, run + 1, 3 * run + 7]


def refill_shape(n):
    """(W, H, frames) whose W * H * frames is n, one chunk: the largest image of at most 8 x 8 pixels, no more than twice as wide as high
    or as high as wide, that divides n (a prime count is one pixel in n frames) -- an image the camera fills with the box, so that the
    paths of a run differ in length"""
    best = (1, 1)
    for h in range(1, 9):
        for w in range(1, 9):
            if n % (w * h) == 0 and 2 * w >= h and 2 * h >= w and w * h > best[0] * best[1]:
                best = (w, h)
    return best[0], best[1], n // (best[0] * best[1])


def _want(name, Ws, Hs, frames, K, Bs, R, cap, mis, power, frame_begin=0, **stripes):
    tris, mats, lights, cam = edge_scene(name)[1]
    gid, frame = do.sample_ids(Ws, Hs, frames, **stripes)
    return (ro.render(tris, mats, Ws, Hs, frame_begin, frames, K, Bs, R, cap, mis=mis, power=power, lights=lights, cam=cam, **stripes),
            ro.samples(tris, mats, Ws, Hs, gid, frame + frame_begin, K, Bs, R, cap, mis=mis, power=power, lights=lights,
                       cam=cam)[0].reshape(frames, -1, 3))


def wanted(name, Ws, Hs, frames, K, Bs, R, cap, mis, power, **kw):
    """the restatement's (framebuffer, radiance [frames, local pixels, 3]) of a case: computed once, shared, read-only"""
    return do.once(_want, name, Ws, Hs, frames, K, Bs, R, cap, bool(mis), bool(power), **kw)


def prefetch(cases):
    """``wanted`` of many cases (tuples of its positional arguments) on threads: the library holds no state"""
    ro.lib()
    with ThreadPoolExecutor(ro.THREADS) as ex:
        list(ex.map(lambda c: wanted(*c), cases))


def parity_cases():
    """every (scene, W, H, frames, K, B, R, cap, mis, power) of the Cornell parity matrix"""
    return [("cornell", W, H, FRAMES, K, B, R, cap, mis, power) for K in KS for R, cap in SETTINGS for mis, power in ESTIMATORS]


def big_cases(which):
    name, K, Bs = which
    return [(name, W, H, FRAMES, K, Bs, R, cap, mis, power) for R, cap in BIG_SETTINGS for mis, power in ESTIMATORS]


def edge_details(edge):
    """(radiance, vertices, end, code, s, q, r) of every sample of an EDGES case (roulette_oracle.samples with details)"""
    name, Ws, Hs, frames, K, Bs, R, cap, mis = EDGES[edge]
    tris, mats, lights, cam = edge_scene(name)[1]
    gid, frame = do.sample_ids(Ws, Hs, frames)
    return ro.samples(tris, mats, Ws, Hs, gid, frame, K, Bs, R, cap, mis=mis, lights=lights, cam=cam, details=True)
