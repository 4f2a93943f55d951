"""Ambient occlusion without a GPU: the ABI of pt_render_ao / pt_occluded_rays, the Python argument checks, and the test-side
restatement (tests/ao_oracle.c) pinned by scenes whose answer is known and by a float64 model."""
import ctypes
import math
import re
import os

import numpy as np
import pytest

import ao_oracle
from conftest import ROOT


def test_ao_params_layout_and_bindings():
    from oclpathtracer_amd import shim

    assert ctypes.sizeof(shim.AoParams) == 64
    offsets = {name: getattr(shim.AoParams, name).offset for name, _ in shim.AoParams._fields_}
    assert offsets == {"width": 0, "height": 4, "frame_begin": 8, "frame_count": 12, "num_triangles": 16, "rays_per_sample": 20,
                       "radius": 24, "miss_value": 28, "stripe_rows": 32, "n_ranks": 36, "rank": 40, "reserved": 44}
    hdr = open(os.path.join(ROOT, "include", "pt_shim.h")).read()
    body = re.search(r"typedef struct pt_ao_params \{(.*?)\} pt_ao_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [n for n, _ in shim.AoParams._fields_]
    lib = ctypes.CDLL(shim.LIB_PATH)
    for name in ("pt_render_ao", "pt_occluded_rays"):
        assert name in shim.SIGNATURES and hasattr(lib, name)


def test_python_argument_checks_come_first():
    from oclpathtracer_amd import adl, scene
    from oclpathtracer_amd.ao import AORenderer
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.query import RayCaster

    tris = np.zeros(2, scene.TRIANGLE_DTYPE)
    # dev=None: any device call would fail differently -- these are refused before one is made
    for kw, err in [(dict(width=0, height=4), ValueError), (dict(width=65536, height=32768), ValueError),
                    (dict(rays_per_sample=0), ValueError), (dict(rays_per_sample=257), ValueError),
                    (dict(radius=0.0), ValueError), (dict(radius=math.inf), ValueError), (dict(radius=math.nan), ValueError),
                    (dict(miss_value=math.nan), ValueError), (dict(stripe_rows=0), ValueError), (dict(rank=1), ValueError),
                    (dict(camera="reference"), TypeError)]:
        args = dict(width=8, height=8)
        args.update(kw)
        W, H = args.pop("width"), args.pop("height")
        with pytest.raises(err):
            AORenderer(None, tris, W, H, **args)
    with pytest.raises(Exception):
        AORenderer(None, tris, 8, 8, camera=Camera(eye=(0, 0, 0), center=(0, 0, 0), up=(0, 1, 0), fov_y_deg=60.0))
    with pytest.raises(TypeError):
        AORenderer(None, np.zeros(3, np.float32), 8, 8)
    with pytest.raises(ValueError):
        AORenderer(None, adl.Buffer(), 8, 8)                  # a buffer needs num_triangles
    rc = RayCaster(None, adl.Buffer(), num_triangles=0)
    with pytest.raises(TypeError):
        rc.occluded(np.zeros((4, 8), np.float32), early_exit=1)
    with pytest.raises(TypeError):
        rc.occluded(np.zeros((4, 7), np.float32), early_exit=True)


def _quad(a, b, c, d):
    """(a, b, c), (c, d, a) as the scene loader pairs them"""
    from oclpathtracer_amd import scene

    t = np.zeros(2, scene.TRIANGLE_DTYPE)
    for k, tri in enumerate(((a, b, c), (c, d, a))):
        for f, p in zip(("p1", "p2", "p3"), tri):
            t[f][k, :3] = p
    return t


def _facing(t, ray_dir):
    """the quad wound so that rays along ray_dir pass the reference's one-sided test (det = dir . cross(e2, e1) > 0)"""
    e1 = t["p2"][:, :3] - t["p1"][:, :3]
    e2 = t["p3"][:, :3] - t["p1"][:, :3]
    if np.dot(np.cross(e2[0], e1[0]), ray_dir) < 0:
        t["p2"], t["p3"] = t["p3"].copy(), t["p2"].copy()
    return t


def test_open_floor_is_never_occluded():
    import ao_oracle
    from oclpathtracer_amd.camera import Camera

    floor = _facing(_quad((-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)), (0, -1, 0))
    cam = Camera(eye=(0.0, 3.0, 0.0), center=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov_y_deg=60.0)
    for radius in (0.05, 1.0, 1e20):
        c = ao_oracle.counts(floor, 16, 16, 0, 2, 8, radius, cam=cam)
        assert c[..., 1].sum() == 16 * 16 * 2
        assert np.array_equal(c[..., 0], 8 * c[..., 1])


def test_closed_box_is_always_occluded():
    import ao_oracle
    from oclpathtracer_amd.camera import Camera

    box = []
    v = lambda x, y, z: (x, y, z)
    for axis in range(3):
        for s in (-1.0, 1.0):
            corners = []
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = [0.0, 0.0, 0.0]
                p[axis] = s
                p[(axis + 1) % 3], p[(axis + 2) % 3] = a, b
                corners.append(v(*p))
            out = np.zeros(3)
            out[axis] = s                                     # rays from inside travel outward through this wall
            box.append(_facing(_quad(*corners), out))
    box = np.concatenate(box)
    # (a primary hit within 0.01 of an edge could start its occlusion ray behind the next wall, GenerateColors.cl:257: the view
    # keeps the hits well inside one wall)
    cam = Camera(eye=(0.1, -0.2, 0.3), center=(0.15, -0.15, -1.0), up=(0.0, 1.0, 0.0), fov_y_deg=40.0)
    c = ao_oracle.counts(box, 16, 12, 0, 2, 6, 1e20, cam=cam)
    assert np.all(c[..., 1] == 2) and np.all(c[..., 0] == 0)


@pytest.mark.parametrize("search,scene,accel", ao_oracle.SLAB_FORMS)
def test_the_slab_scenes_are_open_and_occluded(search, scene, accel):
    """the unbounded scenes of tests/test_gpu_ao.py take their search unbounded, and on at least 0.3 of the pixels a sample hits and
    one of its rays is open (measured: 0.64 - 0.66; on 0.39 - 0.41 of them a ray is occluded as well)"""
    import lit_cells as lc
    from scenes import edge_scene

    tris = edge_scene(scene)[1][0]
    assert lc.form_of(tris, 0, accel)[:2] == (search, False)
    c = ao_oracle.slab_counts(scene)
    opened, hits = c[..., 0], c[..., 1]
    both = ((opened > 0) & (hits > 0)).mean()
    partly = ((opened > 0) & (opened < ao_oracle.SLAB_K * hits)).mean()
    print("%s: open and hits non-zero on %.2f of the pixels, partly occluded on %.2f" % (scene, both, partly))
    assert both >= 0.3 and partly > 0


def test_restatement_agrees_with_a_float64_model(cornell):
    """The occluded / open decisions of tests/ao_oracle.c against tests/f64_model.py's camera, RNG and intersectWorld in float64,
    over the AO rays of a 32 x 32 x 2-frame Cornell render: the float32 and float64 paths part only at near-ties."""
    import ao_oracle
    import f64_model as m

    tris, _ = cornell
    W = H = 32
    K, radius = 8, 0.5
    gid = np.tile(np.arange(W * H, dtype=np.int64), 2)
    frame = np.repeat(np.arange(2, dtype=np.int64), W * H)
    hit32, open32 = ao_oracle.decisions(tris, W, H, gid, frame, K, radius)

    P1 = tris["p1"][:, :3].astype(np.float64)
    E1 = tris["p2"][:, :3].astype(np.float64) - P1
    E2 = tris["p3"][:, :3].astype(np.float64) - P1
    seed = (gid.astype(np.uint64) + m.hash_u32(frame.astype(np.uint64))) & np.uint64(0xFFFFFFFF)
    o, d, seed = m.generate_ray(gid % W, gid // W, W, H, seed)
    idx, t, u, v, _ = m.intersect_world(o, d, P1, E1, E2, None)
    hit = idx >= 0
    p = o + d * t[:, None]
    N = np.cross(E2, E1)[np.maximum(idx, 0)]
    n = N / np.linalg.norm(N, axis=1)[:, None]
    n = np.where((np.sum(n * d, axis=1) < 0.0)[:, None], n, -n)
    axis = np.where((np.abs(n[:, 0]) > 0.001)[:, None], np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))
    tv = np.cross(axis, n)
    tv /= np.linalg.norm(tv, axis=1)[:, None]
    sv = np.cross(n, tv)
    open64 = np.zeros((len(gid), K), np.uint8)
    for k in range(K):
        seed, r1 = m.random_float(seed)
        seed, r2 = m.random_float(seed)
        phi = m.TWO_PI * r1
        wi = sv * (np.cos(phi) * np.sqrt(r2))[:, None] + tv * (np.sin(phi) * np.sqrt(r2))[:, None] + n * np.sqrt(1.0 - r2)[:, None]
        wi /= np.linalg.norm(wi, axis=1)[:, None]
        o2 = p + 0.01 * wi
        j, t2, _, _, _ = m.intersect_world(o2, wi, P1, E1, E2, None)
        open64[:, k] = ~((j >= 0) & (t2 < radius))
    both = hit & (hit32 == 1)
    assert (hit == (hit32 == 1)).mean() > 0.999
    agree = (open32[both] == open64[both]).mean()
    assert both.sum() * K > 10000 and agree >= 0.999, agree
