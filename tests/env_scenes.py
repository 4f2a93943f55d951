"""Scenes and sky maps of the environment-lighting tests (tests/test_env_cpu.py, tests/test_gpu_env.py, tools/env_rates.py): rooms the
sky can look into -- the Cornell room without its ceiling, with and without its panel, the room of many emitters without its ceiling
(518 triangles: the LBVH; 298: the tiled brute force), a single diffuse floor quad -- and the maps.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from oclpathtracer_amd import scene as _scene
from oclpathtracer_amd.camera import Camera
from ris_scenes import many_lights_lbvh, many_lights_tiled
from scenes import edge_scene

CEILING = (0, 1)     # the Cornell room's ceiling
PANEL = (10, 11)     # and its light
SUN_SIZE = 64
SUN_TEXELS = ((35, 38), (35, 39), (36, 38), (36, 39))   # (row, col): four adjacent texels a little off the zenith, towards +x and +z
SUN_RADIANCE, SKY = 5000.0, 0.45
FLOOR_ALBEDO = 0.5
_MADE = {}


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _without(tris, drop):
    keep = np.ones(len(tris), bool)
    keep[list(drop)] = False
    return np.ascontiguousarray(tris[keep])


def floor_quad():
    """(tris, mats, lights, camera): one diffuse quad of albedo 0.5 in the plane y = 0, 100 x 100, wound as the Cornell floor is, seen from
    above at an angle; nothing else, no emitter.  Under a constant sky Le every point of it has the radiance albedo * Le."""
    tris = np.zeros(2, _scene.TRIANGLE_DTYPE)
    tris["p1"][0, :3], tris["p2"][0, :3], tris["p3"][0, :3] = (-50, 0, 50), (50, 0, 50), (50, 0, -50)
    tris["p1"][1, :3], tris["p2"][1, :3], tris["p3"][1, :3] = (50, 0, -50), (-50, 0, -50), (-50, 0, 50)
    tris["id"] = 0
    mats = np.zeros(1, _scene.MATERIAL_DTYPE)
    mats["albedo"][0] = (FLOOR_ALBEDO, FLOOR_ALBEDO, FLOOR_ALBEDO, 1.0)
    mats["emissive"][0, 3] = 1.0
    mats["roughness"], mats["type"] = 1.0, _scene.DIFFUSE
    return tris, mats, np.zeros(0, np.int32), Camera((0.0, 3.0, 4.0), (0.0, 0.0, 0.0))


def env_scene(name):
    """(tris, mats, lights or None, camera or None) of a named scene, each built once: open (the Cornell room without ceiling and panel:
    no emitter), open_panel (without the ceiling only), many_open (ris_scenes.many_lights_lbvh() without the ceiling, 518 triangles),
    many_tiled_open (many_lights_tiled() without it, 298), floor, below (the open room seen from under the horizon: a look-at camera
    outside that looks up), glossy (scenes.glossy_room(0), whose paths go NaN), other_type (a material that is neither type), empty"""
    if name not in _MADE:
        if name == "open":
            tris, mats = _scene.load_model()
            sc = (_without(tris, CEILING + PANEL), mats.copy(), np.zeros(0, np.int32), None)
        elif name == "open_panel":
            tris, mats = _scene.load_model()
            sc = (_without(tris, CEILING), mats.copy(), None, None)
        elif name == "many_open":
            tris, mats = many_lights_lbvh()
            sc = (_without(tris, CEILING), mats.copy(), None, None)
            assert len(sc[0]) >= 512
        elif name == "many_tiled_open":
            tris, mats = many_lights_tiled()
            sc = (_without(tris, CEILING), mats.copy(), None, None)
            assert 257 <= len(sc[0]) <= 511
        elif name == "floor":
            sc = floor_quad()
        elif name == "below":
            tris, mats, lights, _ = env_scene("open_panel")
            sc = (tris, mats, lights, Camera((0.0, -3.0, 6.0), (0.0, 4.0, -3.0)))
        elif name == "glossy":
            sc = edge_scene("glossy:0")[1]
        elif name == "other_type":
            sc = edge_scene("other_type")[1]
        elif name == "empty":
            _, mats = _scene.load_model()
            sc = (np.zeros(0, _scene.TRIANGLE_DTYPE), mats.copy(), np.zeros(0, np.int32), None)
        else:
            raise KeyError(name)
        _MADE[name] = _freeze(*sc)
    return _MADE[name]


def env_map(name):
    """float32 [N, N, 4] of a named map, each built once: grey:N (every texel 0.45), gradient:N (a distinct value per texel and channel),
    sun (SUN_TEXELS of 5 000 on a sky of 0.45, N = 64), zero:N, bad:16 (the gradient with a NaN texel, two negative ones, an infinite component and
    one of -0, where the open room's rays look)"""
    key = "map:" + name
    if key not in _MADE:
        kind, _, arg = name.partition(":")
        N = int(arg) if arg else SUN_SIZE
        t = np.zeros((N, N, 4), np.float32)
        if kind == "grey":
            t[..., :3] = SKY
        elif kind == "gradient":
            i = np.arange(N * N, dtype=np.float64).reshape(N, N)
            t[..., 0] = 0.25 + i / (N * N)
            t[..., 1] = 1.25 - i / (N * N)
            t[..., 2] = 0.5 + (i % 7) / 8.0
        elif kind == "sun":
            t[..., :3] = SKY
            for r, c in SUN_TEXELS:
                t[r, c, :3] = SUN_RADIANCE
        elif kind == "zero":
            pass
        elif kind == "bad":
            assert N == 16, "the texels are placed where the open room's rays look"
            t = env_map("gradient:16").copy()
            flat = t.reshape(-1, 4)
            flat[59, :3] = np.nan                          # seen by primary rays above the back wall
            flat[52, :3] = flat[218, :3] = (-1.0, -2.0, -0.5)   # by primary rays, and by rays that leave through the open ceiling
            flat[228, 0] = np.inf
            flat[212, 1] = -0.0
        else:
            raise KeyError(name)
        t[..., 3] = 1.0
        _MADE[key] = _freeze(t)[0]
    return _MADE[key]
