"""Scenes and light lists of the light-choice-by-power tests (tests/test_power_cpu.py, tests/test_gpu_power.py), beside those of
scenes.py.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from oclpathtracer_amd import scene as _scene

SMALL, TINY = 48, 8          # the dim emitters of unequal_lights: q of a few units; and the ones whose q is the floor, 1
WALL = 3                     # a triangle of the Cornell box that emits nothing
_UNEQUAL = []


def unequal_lights():
    """(tris, mats): the Cornell room with its panel (triangles 10 and 11, emission 30) plus SMALL small dim emissive triangles
    (emission 1, a new material), TINY more whose power is below 1 / 65536 of a panel triangle's (emission 1e-4: q = 1), and one
    emissive triangle of no area (q = 0) -- 36 + 48 + 8 + 1 = 93 triangles, ``scene.emitters`` names the last 57 and the panel."""
    if not _UNEQUAL:
        tris, mats = _scene.load_model()
        rng = np.random.default_rng(7)
        n = SMALL + TINY + 1
        extra = np.zeros(n, _scene.TRIANGLE_DTYPE)
        c = rng.uniform([-2.3, 0.4, -5.0], [2.3, 4.9, -0.8], (n, 3)).astype(np.float32)
        extra["p1"][:, :3] = c
        extra["p2"][:, :3] = c + rng.uniform(-0.12, 0.12, (n, 3)).astype(np.float32)
        extra["p3"][:, :3] = c + rng.uniform(-0.12, 0.12, (n, 3)).astype(np.float32)
        extra["p2"][-1] = extra["p3"][-1] = extra["p1"][-1]                  # no area
        more = np.zeros(2, _scene.MATERIAL_DTYPE)
        more["albedo"][:, :3] = 0.5
        more["albedo"][:, 3] = more["emissive"][:, 3] = 1.0
        more["roughness"], more["type"] = 1.0, _scene.DIFFUSE
        more["emissive"][0, :3], more["emissive"][1, :3] = 1.0, 1e-4
        extra["id"] = len(mats)
        extra["id"][SMALL:SMALL + TINY] = len(mats) + 1
        _UNEQUAL.append((np.concatenate([tris, extra]), np.concatenate([mats, more])))
        for a in _UNEQUAL[0]:
            a.setflags(write=False)
    return _UNEQUAL[0]


def edge_list():
    """int32: a list over unequal_lights() made for the edges of the choice -- a panel triangle first and (again: its count is 2) last,
    a wall (q = 0) directly before the other panel triangle, every q = 1 triangle twenty times over, the small ones, the one of no
    area; unsorted, with duplicates and a non-emitter"""
    tiny = np.tile(np.arange(36 + SMALL, 36 + SMALL + TINY), 20)
    return np.concatenate([[10, WALL, 11], tiny, np.arange(36, 36 + SMALL)[::-1], [36 + SMALL + TINY, WALL, 10]]).astype(np.int32)


def zero_list():
    """int32: entries of unequal_lights() none of which has positive power: walls and the emitter of no area (total == 0)"""
    return np.array([WALL, 0, 36 + SMALL + TINY, WALL], np.int32)
