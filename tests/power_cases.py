"""The inputs of tests/test_gpu_power.py and what the restatement (tests/power_oracle.c) says of them: one table, so that
tests/test_power_cpu.py proves its floors on exactly the scenes, lists and sizes the device renders.  TEST INFRASTRUCTURE.

A case is (mode of power_oracle, scene name, list name or None = scene.emitters, W, H, frames, K, B, stripes)."""
from __future__ import annotations

import numpy as np

import direct_oracle as do
import power_oracle as po
import power_scenes as ps
from indirect_edges import clamped_raw
from scenes import edge_scene

MODES = (po.DIRECT, po.INDIRECT, po.MIS)
MODE_NAMES = {po.DIRECT: "direct", po.INDIRECT: "indirect", po.MIS: "mis"}
W, H, FRAMES = 40, 24, 3
SEARCH_KB = (2, 4)                                              # (K, B) of the cases rendered under every search
BIG = ("nested:10", "nested:15")                                # the tiled table; the LBVH and forced brute force: 20 and 30 unequal emitters
BIG_KB = (2, 3)
EDGE_KB = (4, 4)                                                # the edge list and the empty table
SMALL = ((1, 1, 16), (5, 3, 4), (13, 5, 4))                     # (W, H, B), 2 frames, K = 4: 1, 15 and 65 pixels
STRIPE_ROWS, RANKS = 4, 3
PARAM_KB = ((1, 4), (256, 1), (1, 1), (2, 24))                  # K = 1 and 256, B = 1 and a deep B


def scene_of(name):
    """(tris, mats, camera or None) of a named scene: "unequal" (power_scenes.unequal_lights) or a name of scenes.edge_scene"""
    if name == "unequal":
        return ps.unequal_lights() + (None,)
    tris, mats, _, cam = edge_scene(name)[1]
    return tris, mats, cam


def lights_of(scene, name):
    """the light list of a case as the restatement takes it: None (the emitters), "edges" / "zero" of power_scenes, or "clamped", what
    the device makes of indirect_edges.clamped_raw"""
    if name is None:
        return None
    if name == "clamped":
        ntri = len(scene_of(scene)[0])
        return np.clip(clamped_raw(ntri), 0, ntri - 1).astype(np.int32)
    return {"edges": ps.edge_list, "zero": ps.zero_list}[name]()


def edge_cases():
    """the inputs rendered for an edge of the choice: (mode, scene, list, W, H, frames, K, B)"""
    return [(m, "unequal", li, W, H, FRAMES) + EDGE_KB for m in MODES for li in ("edges", "zero")]


def _want(mode, scene, lights, Ws, Hs, frames, K, B, **stripes):
    tris, mats, cam = scene_of(scene)
    li = lights_of(scene, lights)
    gid, frame = do.sample_ids(Ws, Hs, frames, **stripes)
    return (po.render(mode, tris, mats, Ws, Hs, 0, frames, K, B, lights=li, cam=cam, **stripes),
            po.samples(mode, tris, mats, Ws, Hs, gid, frame, K, B, lights=li, cam=cam).reshape(frames, -1, 3))


def wanted(mode, scene, lights, Ws, Hs, frames, K, B, **stripes):
    """the restatement's (framebuffer, radiance [frames, local pixels, 3]) of a case: computed once, shared, read-only"""
    return do.once(_want, mode, scene, lights, Ws, Hs, frames, K, B, **stripes)


def details(mode, scene, lights, Ws, Hs, frames, K, B):
    """po.samples(details=True) of every sample of a case, and the list"""
    tris, mats, cam = scene_of(scene)
    li = lights_of(scene, lights)
    gid, frame = do.sample_ids(Ws, Hs, frames)
    return po.samples(mode, tris, mats, Ws, Hs, gid, frame, K, B, lights=li, cam=cam, details=True), li
