"""The inputs of tests/test_gpu_power.py and tests/test_gpu_light_scale.py and what the restatements (tests/power_oracle.c, and for the
uniform choice direct_oracle.c, indirect_oracle.c and mis_oracle.c) say of them: one table, so that tests/test_power_cpu.py proves its
floors on exactly the scenes, lists and sizes the device renders.  TEST INFRASTRUCTURE.

A case is (mode of power_oracle, scene name, list name or None = scene.emitters, W, H, frames, K, B, stripes).  The lists of LONG_LISTS
have up to 2^24 - 1 entries: their table and counts are made once (``table_of``) and handed to every restatement call."""
from __future__ import annotations

import numpy as np

import direct_oracle as do
import indirect_oracle as io
import mis_oracle as mo
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
# lists over the unequal lights whose total passes 2^32: ps.LONG entries (257 tiles), and the two of ps.MAX entries
LONG_LISTS = {"long": lambda: ps.long_list(ps.LONG), "max": lambda: ps.long_list(ps.MAX), "panels": ps.panel_list}
LONG_KB = (4, 4)                                                # every render of a long list; 3 frames of "long", MAX_FRAMES of the others
LONG_SMALL = (13, 5)                                            # the small image of "long"
MAX_FRAMES = 2


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
    return {"edges": ps.edge_list, "zero": ps.zero_list, **LONG_LISTS}[name]()


def _table(scene, lights):
    tris, mats, _ = scene_of(scene)
    li = lights_of(scene, lights)
    return po.table(tris, mats, li) + (mo.light_counts(li, len(tris)),)


def table_of(scene, lights):
    """the restatement's (cdf, tri_q, counts) of a named list: computed once, shared, read-only"""
    return do.once(_table, scene, lights)


def _given(scene, lights):
    """the table and the counts as keywords of a power_oracle call: made once for a list of LONG_LISTS, left to the call otherwise"""
    if lights not in LONG_LISTS:
        return {}
    cdf, tri_q, counts = table_of(scene, lights)
    return dict(tab=(cdf, tri_q), counts=counts)


def edge_cases():
    """the inputs rendered for an edge of the choice: (mode, scene, list, W, H, frames, K, B)"""
    return [(m, "unequal", li, W, H, FRAMES) + EDGE_KB for m in MODES for li in ("edges", "zero")]


def _want(mode, scene, lights, Ws, Hs, frames, K, B, **stripes):
    tris, mats, cam = scene_of(scene)
    li = lights_of(scene, lights)
    gid, frame = do.sample_ids(Ws, Hs, frames, **stripes)
    kw = _given(scene, lights)
    return (po.render(mode, tris, mats, Ws, Hs, 0, frames, K, B, lights=li, cam=cam, **kw, **stripes),
            po.samples(mode, tris, mats, Ws, Hs, gid, frame, K, B, lights=li, cam=cam, **kw).reshape(frames, -1, 3))


def wanted(mode, scene, lights, Ws, Hs, frames, K, B, **stripes):
    """the restatement's (framebuffer, radiance [frames, local pixels, 3]) of a case: computed once, shared, read-only"""
    return do.once(_want, mode, scene, lights, Ws, Hs, frames, K, B, **stripes)


def details(mode, scene, lights, Ws, Hs, frames, K, B):
    """po.samples(details=True) of every sample of a case, and the list"""
    tris, mats, cam = scene_of(scene)
    li = lights_of(scene, lights)
    gid, frame = do.sample_ids(Ws, Hs, frames)
    return po.samples(mode, tris, mats, Ws, Hs, gid, frame, K, B, lights=li, cam=cam, details=True, **_given(scene, lights)), li


def _want_uniform(mode, scene, lights, Ws, Hs, frames, K, B):
    tris, mats, cam = scene_of(scene)
    li = lights_of(scene, lights)
    gid, frame = do.sample_ids(Ws, Hs, frames)
    if mode == po.DIRECT:
        fb, rad = do.render(tris, mats, Ws, Hs, 0, frames, K, lights=li, cam=cam), do.decisions(tris, mats, Ws, Hs, gid, frame, K, lights=li, cam=cam)[2]
    elif mode == po.INDIRECT:
        fb, rad = io.render(tris, mats, Ws, Hs, 0, frames, K, B, lights=li, cam=cam), io.samples(tris, mats, Ws, Hs, gid, frame, K, B, lights=li, cam=cam)[0]
    else:
        kw = dict(lights=li, cam=cam, counts=table_of(scene, lights)[2] if lights in LONG_LISTS else None)
        fb, rad = mo.render(tris, mats, Ws, Hs, 0, frames, K, B, **kw), mo.samples(tris, mats, Ws, Hs, gid, frame, K, B, **kw)[0]
    return fb, rad.reshape(frames, -1, 3)


def wanted_uniform(mode, scene, lights, Ws, Hs, frames, K, B):
    """``wanted`` for the uniform choice: the parents' restatements (direct_oracle, indirect_oracle, mis_oracle) of the same case"""
    return do.once(_want_uniform, mode, scene, lights, Ws, Hs, frames, K, B)
