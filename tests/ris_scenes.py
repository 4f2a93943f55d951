"""Scenes of the resampled-light-sampling tests (tests/test_ris_cpu.py, tests/test_gpu_ris.py, tools/ris_rates.py), beside those of
scenes.py and power_scenes.py: a room lit by many small emitters of equal power, where the choice by power is the uniform choice and
only a choice that looks at the shading point helps.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from oclpathtracer_amd import scene as _scene
from power_scenes import edge_list, unequal_lights, zero_list
from scenes import MIXED_SCALE, edge_scene

GRID = 8                     # GRID x GRID emitters
SIDE, PITCH = 0.25, 0.625    # an emitter's legs and the grid's pitch: multiples of 2^-3, so every coordinate and both edges are exact
X0, Y, Z0 = -2.25, 5.25, -0.5   # the first emitter's corner; the ceiling is at y = 5.488
EMISSION = 20.0
PANEL_MATERIAL = 5           # the Cornell box's own panel (triangles 10 and 11), switched off here
_MADE = {}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def many_lights():
    """(tris, mats): the Cornell room with its panel's emission set to 0 and, below the ceiling, GRID x GRID = 64 small emissive
    triangles of bit-equal area and emission, facing down (N = cross(e2, e1) points up, as the panel's does), on a regular grid -- 100
    triangles.  ``scene.emitters`` names the 64: a power of two of entries of equal power, so every q is 65536 and the table is the
    uniform choice exactly."""
    if "many" not in _MADE:
        tris, mats = _scene.load_model()
        mats = mats.copy()
        mats["emissive"][PANEL_MATERIAL, :3] = 0.0
        n = GRID * GRID
        extra = np.zeros(n, _scene.TRIANGLE_DTYPE)
        i, j = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
        cx = (X0 + PITCH * i.reshape(-1)).astype(np.float32)
        cz = (Z0 - PITCH * j.reshape(-1)).astype(np.float32)
        y = np.full(n, Y, np.float32)
        extra["p1"][:, :3] = np.stack([cx, y, cz], 1)
        extra["p2"][:, :3] = np.stack([cx, y, cz - np.float32(SIDE)], 1)
        extra["p3"][:, :3] = np.stack([cx + np.float32(SIDE), y, cz - np.float32(SIDE)], 1)
        more = np.zeros(1, _scene.MATERIAL_DTYPE)
        more["albedo"][:, :3] = 0.5
        more["albedo"][:, 3] = more["emissive"][:, 3] = 1.0
        more["roughness"], more["type"] = 1.0, _scene.DIFFUSE
        more["emissive"][0, :3] = EMISSION
        extra["id"] = len(mats)
        _MADE["many"] = _freeze(np.concatenate([tris, extra]), np.concatenate([mats, more]))
    return _MADE["many"]


def _with_filler(count, key):
    """many_lights() and ``count`` small triangles that emit nothing behind the camera (z in [8, 16], the eye is at z = 4 and looks
    down -z): no primary ray sees them; a path that leaves the room through its open front may"""
    if key not in _MADE:
        tris, mats = many_lights()
        rng = np.random.default_rng(23)
        fill = np.zeros(count, _scene.TRIANGLE_DTYPE)
        c = rng.uniform([-4.0, 0.0, 8.0], [4.0, 6.0, 16.0], (count, 3)).astype(np.float32)
        fill["p1"][:, :3] = c
        fill["p2"][:, :3] = c + rng.uniform(-0.2, 0.2, (count, 3)).astype(np.float32)
        fill["p3"][:, :3] = c + rng.uniform(-0.2, 0.2, (count, 3)).astype(np.float32)
        fill["id"] = 0
        _MADE[key] = _freeze(np.concatenate([tris, fill])) + (mats,)
    return _MADE[key]


def many_lights_lbvh():
    """many_lights() with 420 filler triangles: 520, PT_OPT_ACCEL 0 takes the LBVH"""
    tris, mats = _with_filler(420, "lbvh")
    assert len(tris) >= 512
    return tris, mats


def many_lights_tiled():
    """many_lights() with 200 filler triangles: 300, the tiled brute-force table (257 .. 511)"""
    tris, mats = _with_filler(200, "tiled")
    assert 257 <= len(tris) <= 511
    return tris, mats


def ris_scene(name):
    """(tris, mats, lights, camera) of a named input of the RIS tests: many, many_lbvh, many_tiled, cornell, unequal (unequal_lights()
    with ``scene.emitters``), edge_list, zero_list (power_scenes' lists over unequal_lights()), out_of_range (many_lights() with light
    indices out of range at either end: they are clamped), scaled (scenes.direct_scaled(10, MIXED_SCALE), 360 triangles with its own
    list and camera: vertices within 0.02 of an emitter, whose shadow rays have tl <= 0)"""
    if name == "many":
        return many_lights() + (None, None)
    if name == "many_lbvh":
        return many_lights_lbvh() + (None, None)
    if name == "many_tiled":
        return many_lights_tiled() + (None, None)
    if name == "cornell":
        return _scene.load_model() + (None, None)
    if name == "unequal":
        return unequal_lights() + (None, None)
    if name == "edge_list":
        return unequal_lights() + (edge_list(), None)
    if name == "zero_list":
        return unequal_lights() + (zero_list(), None)
    if name == "scaled":
        return edge_scene("scaled:10,%d" % MIXED_SCALE)[1]
    if name == "out_of_range":
        tris, mats = many_lights()
        li = _scene.emitters(tris, mats).astype(np.int32).copy()
        li[::5] = -1 - li[::5]            # clamped to triangle 0, a wall
        li[3::7] = len(tris) + li[3::7]   # clamped to the last triangle, an emitter
        return tris, mats, li, None
    raise KeyError(name)
