"""Scenes of the indirect-illumination tests (tests/test_indirect_cpu.py, tests/test_gpu_indirect.py), beside those of scenes.py.
TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from oclpathtracer_amd import scene as _scene
from scenes import nested_boxes


def diffuse_cornell():
    """The Cornell box with every GGX material made diffuse (albedo and emission kept).  Light sampling without multiple
    importance sampling loses nothing on a diffuse surface but variance; on the box's roughness-0.008 GGX surfaces next to the
    light it is too noisy for a statistical comparison."""
    tris, mats = _scene.load_model()
    mats = mats.copy()
    glossy = mats["type"] == _scene.SPECULAR
    assert glossy.any()
    mats["type"][glossy] = _scene.DIFFUSE
    return tris, mats


def lbvh_boxes():
    """nested_boxes(15), 540 triangles: PT_OPT_ACCEL 0 takes the LBVH (direct illumination's lbvh_scene)"""
    tris, mats = nested_boxes(15)
    assert len(tris) >= 512
    return tris, mats


def tiled_boxes():
    """nested_boxes(10), 360 triangles: the tiled brute-force table (257 .. 511)"""
    tris, mats = nested_boxes(10)
    assert 257 <= len(tris) <= 511
    return tris, mats
