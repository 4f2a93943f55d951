"""The inputs of tests/test_gpu_mis.py and what the restatement (tests/mis_oracle.c) says of them: one table, so that
tests/test_mis_cpu.py proves its floors on exactly the scenes, lists and sizes the device renders.  TEST INFRASTRUCTURE.

A case is (scene name of scenes.edge_scene, list name of LISTS or None = scene.emitters, W, H, frames, K, B, stripes): ``stripes`` a
dict of stripe_rows / n_ranks / rank."""
from __future__ import annotations

import numpy as np

import direct_oracle as do
import mis_oracle as mo
from indirect_edges import clamped_raw
from scenes import edge_scene

W, H, FRAMES = 40, 24, 3
SEARCH_KB = ((1, 16), (4, 4))                                   # (K, B) of the cases rendered under every search
PARAM_KB = tuple((K, B) for K in (1, 4) for B in (1, 2, 4, 16))
FINITE = (("finite:5", 2, 6), ("finite:8", 2, 6))               # (scene, K, B)
BIG = (("nested:10", 2, 4), ("nested:15", 2, 4))                # the tiled table; the LBVH and forced brute force
SMALL = ((1, 1, 16), (5, 3, 4), (13, 5, 4))                     # (W, H, B), 2 frames, K = 4: 1, 15 and 65 pixels
SMALL_SCENES = ("cornell", "nested:15")
STRIPE_ROWS, RANKS = 4, 3
# light lists of the Cornell box (emitters 10 and 11, triangle 3 a wall)
LISTS = {"emitters": (10, 11), "duplicated": (10, 11, 10), "missing": (10,), "wall": (10, 11, 3), "unsorted": (11, 3, 10, 10)}
LIST_KB = (2, 4)


def cases():
    """every (scene, list, W, H, frames, K, B, stripes) the GPU module compares with the restatement"""
    out = [("cornell", None, W, H, FRAMES, K, B, {}) for K, B in PARAM_KB]
    out += [("cornell", None, W, H, FRAMES, K, B, {}) for K, B in SEARCH_KB if (K, B) not in PARAM_KB]
    out += [(name, None, W, H, FRAMES, K, B, {}) for name, K, B in FINITE + BIG]
    out += [(name, None, Ws, Hs, 2, 4, B, {}) for name in SMALL_SCENES for Ws, Hs, B in SMALL]
    out += [("cornell", None, W, H, 2, 1, 4, dict(stripe_rows=STRIPE_ROWS))]
    out += [("cornell", None, W, H, 2, 1, 4, dict(stripe_rows=STRIPE_ROWS, n_ranks=RANKS, rank=r)) for r in range(RANKS)]
    out += [("cornell", None, W, H, 2 * FRAMES, 1, 4, {})]       # two calls of three frames
    out += [("cornell", name, W, H, FRAMES) + LIST_KB + ({},) for name in LISTS]
    out += [("cornell", "clamped", W, H, FRAMES) + LIST_KB + ({},)]
    return out


def lights_of(scene, name):
    """the light list of a case as the restatement takes it: None (the emitters), a list of LISTS, or the clamped form of
    indirect_edges.clamped_raw (what the device makes of the raw list)"""
    if name is None:
        return None
    ntri = len(edge_scene(scene)[1][0])
    if name == "clamped":
        return np.clip(clamped_raw(ntri), 0, ntri - 1).astype(np.int32)
    return np.asarray(LISTS[name], np.int32)


def _want(scene, lights, Ws, Hs, frames, K, B, **stripes):
    tris, mats, _, cam = edge_scene(scene)[1]
    li = lights_of(scene, lights)
    gid, frame = do.sample_ids(Ws, Hs, frames, **stripes)
    return (mo.render(tris, mats, Ws, Hs, 0, frames, K, B, lights=li, cam=cam, **stripes),
            mo.samples(tris, mats, Ws, Hs, gid, frame, K, B, lights=li, cam=cam)[0].reshape(frames, -1, 3))


def wanted(scene, lights, Ws, Hs, frames, K, B, **stripes):
    """the restatement's (framebuffer, radiance [frames, local pixels, 3]) of a case: computed once, shared, read-only"""
    return do.once(_want, scene, lights, Ws, Hs, frames, K, B, **stripes)


def details(scene, lights, Ws, Hs, frames, K, B, **stripes):
    """mo.details of every local sample of a case"""
    tris, mats, _, cam = edge_scene(scene)[1]
    gid, frame = do.sample_ids(Ws, Hs, frames, **stripes)
    return mo.details(tris, mats, Ws, Hs, gid, frame, K, B, lights=lights_of(scene, lights), cam=cam)
