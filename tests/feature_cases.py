"""The inputs of the first-hit feature tests: (triangles, materials, camera or None) of a named case, each built once, and the oracle's
samples of a case, computed once and shared.  TEST INFRASTRUCTURE, shared by tests/test_features_cpu.py (which proves that each input
reaches its edge, on the oracle alone) and tests/test_gpu_features.py (which renders them).  Everything is generated from fixed seeds.
"""
from __future__ import annotations

import numpy as np

import feature_oracle as fo
import reference_cases
import scenes
from oclpathtracer_amd import scene as _scene
from oclpathtracer_amd.camera import Camera

W, H = 40, 24   # 960 pixels: 15 full waves
SLAB_W, SLAB_H = 24, 16
SLAB_FORMS = (("lds", "slab:1", 1), ("tiled", "slab:10", 1), ("lbvh", "slab:15", 0))   # (search, case, PT_OPT_ACCEL): lit_cells' slab forms



def soup_camera():
    """a camera that looks at the middle of the soups (scenes.soup, scenes.with_big: triangles in [-3, 3]^3) from outside them.  (Made
    on demand: a Camera loads the library, which a module must not do while it is imported -- torch has to come first.)"""
    return Camera(eye=(0.5, 0.25, 7.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_y_deg=50.0)


LENS_R, LENS_F = 0.05, 6.0

BELOW, ABOVE = -5, 99   # material ids outside every table of this file


def odd_materials():
    """reference_cases.odd_materials -- NaN, negative and zero albedo, types 0 and 3 -- with the ids of the four triangles the
    reference camera sees most of set to: one above the table and one below 0, which the clamp of pt_render_features takes to the
    last material and to material 0; 12, the NaN albedo; 1, the negative one"""
    tris, mats = reference_cases.odd_materials()
    tris = tris.copy()
    seen = fo.samples(tris, mats, W, H, 1).tri   # which triangles the reference camera's frame 0 meets, most samples first
    order = [int(t) for t in np.argsort(-np.bincount(seen[seen >= 0], minlength=len(tris))) if (seen == t).any()]
    assert len(order) >= 4
    tris["id"][order[0]] = ABOVE
    tris["id"][order[1]] = BELOW
    tris["id"][order[2]] = 12   # the NaN albedo
    tris["id"][order[3]] = 1    # the negative one
    return tris, mats


def overflowing_triangle():
    """One triangle of edges 2.5e19 close in front of the reference camera, tilted by 60 degrees: its det and t are finite, but the y
    component of cross(e2, e1) overflows to infinity, dot(N, N) is infinite, 1 / sqrt is 0 and the HitRecord normal is (0, NaN, -0)"""
    a = np.float32(2.5e19)
    th = np.deg2rad(60.0)
    t = np.zeros(1, _scene.TRIANGLE_DTYPE)
    p1 = np.array([-0.3, 2.45, 3.2], np.float32)
    t["p1"][0, :3] = p1
    t["p2"][0, :3] = p1 + np.array([a, 0.0, 0.0], np.float32)
    t["p3"][0, :3] = p1 + np.array([0.0, a * np.cos(th), a * np.sin(th)], np.float32)
    t["id"] = 3
    return t


def non_finite():
    """The Cornell box, scenes.non_finite(200) and overflowing_triangle().  A triangle with a NaN or an infinity in p1 is never hit --
    its t is NaN and `t > 0` fails (:125) --, so scenes.non_finite alone gives no NaN record: its triangles are what the search must
    pass over, and the NaN records come from the one finite triangle whose normal overflows."""
    tris, mats = _scene.load_model()
    return np.concatenate([tris, scenes.non_finite(200), overflowing_triangle()]), mats


_CASES = {}


def case(name):
    """(tris, mats, camera) of cornell, odd_materials, other_type, from_behind, non_finite, soup, with_big, lens, empty, slab:COPIES (an
    unbounded scene that shades: scenes.slab)"""
    if name not in _CASES:
        box, mats = _scene.load_model()
        if name == "cornell":
            c = (box, mats, None)
        elif name == "odd_materials":
            c = odd_materials() + (None,)
        elif name == "other_type":
            c = scenes.direct_other_type()[:2] + (None,)
        elif name == "from_behind":
            t, m, _, cam = scenes.direct_from_behind()
            c = (t, m, cam)
        elif name == "non_finite":
            c = non_finite() + (None,)
        elif name == "soup":
            c = (scenes.soup(2000), mats, soup_camera())
        elif name == "with_big":
            c = (scenes.with_big(64), mats, soup_camera())   # (PT_BVH_BIG_MAX: the table of big triangles is full)
        elif name == "lens":
            ref = Camera.reference()
            c = (box, mats, Camera(eye=ref.eye, center=ref.center, up=ref.up, fov_y_deg=ref.fov_y_deg, lens_radius=LENS_R, focus_distance=LENS_F))
        elif name == "empty":
            c = (box[:0].copy(), mats, None)
        elif name.startswith("slab:"):
            t, m, _, cam = scenes.edge_scene(name)[1]
            c = (t, m, cam)
        else:
            raise ValueError(name)
        _CASES[name] = c
    return _CASES[name]


def oracle(name, w=W, h=H, frames=2, frame_begin=0, **stripes) -> fo.Samples:
    """the oracle's samples of a case, once per (case, shape, frames, stripes), read-only"""
    tris, mats, cam = case(name)
    key = (name, w, h, frames, frame_begin, tuple(sorted(stripes.items())))
    return fo.once(key, lambda: fo.samples(tris, mats, w, h, frames, frame_begin=frame_begin, cam=cam, **stripes))
