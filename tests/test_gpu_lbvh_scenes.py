"""What the LBVH takes as candidates, at the edges: the scale, offset and shape of the scene, the builder's boundaries -- queries
under PT_OPT_ACCEL = 2 against the CPU oracle and against PT_OPT_ACCEL = 1, bit for bit -- and an independent check of every
hierarchy the device built (pt_bvh_snapshot, tests/bvh_check.py): structure, containment of every triangle below every box,
tightness.  The scenes are tests/scenes.py's; the oracle's scale identities they lean on are tests/test_lbvh_scale_cpu.py's."""
import ctypes

import numpy as np
import pytest

import bvh_check as B
import query_oracle as qo
import scenes as S
from gpu_support import assert_hits_equal, options
from oclpathtracer_amd import shim

pytestmark = pytest.mark.gpu


def snapshot(device):
    """(records uint8 [R, 64], grid_min, grid_step, big indices) of the LBVH that stands for the device's prepared scene"""
    lib = shim.load()
    info = shim.BvhInfo()
    shim.check(lib.pt_bvh_snapshot(device._h, ctypes.byref(info), None, 0, None))
    recs = np.zeros((info.records, 64), np.uint8)
    big = np.zeros(shim.PT_BVH_SNAPSHOT_BIG_MAX, np.int32)
    shim.check(lib.pt_bvh_snapshot(device._h, ctypes.byref(info), recs.ctypes.data_as(ctypes.c_void_p), len(recs), big.ctypes.data_as(ctypes.c_void_p)))
    assert info.records == len(recs) and 0 <= info.num_big <= shim.PT_BVH_SNAPSHOT_BIG_MAX
    return recs, np.array(info.grid_min[:], np.float32), np.array(info.grid_step[:], np.float32), big[: info.num_big].copy(), info.num_triangles


def check_hierarchy(device, tris, what):
    """snapshot the hierarchy that stands and hand it to the checker; the snapshot itself must change nothing"""
    lib = shim.load()
    builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
    ws = device.getWorkspaceMemory()
    recs, gmin, gstep, big, ntri = snapshot(device)
    again = snapshot(device)
    assert ntri == len(tris)
    assert np.array_equal(recs, again[0]) and np.array_equal(big, again[3]), what + ": two snapshots differ"
    assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds and device.getWorkspaceMemory() == ws
    print(what, end=": ")
    return B.check(tris, recs, gmin, gstep, big)


def _probe_rays(n=64):
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = np.random.default_rng(1).uniform(-4, 4, (n, 3))
    r[:, 3], r[:, 4:7] = 1e20, np.random.default_rng(2).normal(size=(n, 3))
    return r


@pytest.mark.parametrize("name", S.NAMES)
def test_scene_through_the_lbvh(device, name):
    from oclpathtracer_amd.query import RayCaster

    tris, rays = S.scene(name)
    want = qo.closest_threads(tris, rays)
    wt = want[:, 1].view(np.int32)
    print("%s: %d triangles, the oracle hits with %d of %d rays" % (name, len(tris), int((wt >= 0).sum()), len(rays)))
    if name in ("shared_point", "none_finite"):
        assert np.all(wt < 0)                                   # nothing can be hit, and nothing may fail
    elif not name.startswith("scale") or int(name[5:]) in S.IDENTITY or name in ("one_finite",):
        assert (wt >= 0).mean() >= 0.2, name + ": a case that hardly hits tests nothing"
    # |e1| |e2| above PT_DET_BOUND_MAX: the shim then takes the exact-division (DET_BOUNDED = false) kernels.  The test can show the
    # precondition (here, with the L1 norms the shim's own bound uses) and the results, not which instantiation ran.
    if name == "slab541" or name.startswith("scale") and int(name[5:]) >= 34:
        e1 = np.abs(tris["p2"][:, :3].astype(np.float64) - tris["p1"][:, :3]).sum(1)
        e2 = np.abs(tris["p3"][:, :3].astype(np.float64) - tris["p1"][:, :3]).sum(1)
        assert (e1 * e2).max() > 2.0e19
    if name == "slab541":                                       # (tests/test_bvh_check_cpu.py has the same conditions without a device)
        hit = wt >= 0
        assert hit.mean() >= 0.5 and (wt[hit] == len(tris) - 1).mean() >= 0.1 and (wt[hit] < len(tris) - 1).mean() >= 0.3
    lib = shim.load()
    count = lambda: lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
    rc = RayCaster(device, tris)
    try:
        if name == "slab541":                                   # its first half is what pt_camera_rays makes of the scene's camera
            cam = S.edge_scene("slab:15")[1][3]
            first = rc.camera_rays(S.SLAB_RAYS_W, S.SLAB_RAYS_H, 0, cam)
            assert np.array_equal(words8(first).view(np.uint32), rays[: len(first)].view(np.uint32)), "pt_camera_rays differs from its restatement"
        if name in ("n511", "n512"):                            # PT_OPT_ACCEL = 0: the hierarchy from 512 triangles on
            with options(device, ACCEL=0):
                b = count()
                auto = rc.closest(rays)
                assert count() - b == (1 if len(tris) >= 512 else 0), name + ": the wrong search ran"
            assert_hits_equal(auto, want, name + " a0")
        with options(device, ACCEL=2):
            b = count()
            got2 = rc.closest(rays)
            occ = rc.occluded(rays)
            early = rc.occluded(rays, early_exit=True)
            assert count() - b == (0 if name == "n512" else 1), name + ": the shim did not take the LBVH"
            check_hierarchy(device, tris, name)
            if name == "slab541":                               # no search was cut short: nothing is deferred to the next observing call
                assert lib.pt_sync(device._h) == shim.PT_OK, lib.pt_last_error()
                assert snapshot(device)[3].tolist() == [len(tris) - 1], "the slab alone is kept out of the hierarchy"
            if name in ("big64", "big65"):                      # the builder's n > PT_BVH_BIG_MAX and k < PT_BVH_BIG_MAX comparisons sit here
                assert len(snapshot(device)[3]) == (64 if name == "big64" else 0), name + ": the scene no longer sits on the boundary"
        with options(device, ACCEL=1):
            got1 = rc.closest(rays)
    finally:
        rc.release()
    bad = np.flatnonzero(got2["tri"] != wt)
    for k in bad[:6]:
        print("  ray %d: origin %r dir %r -> oracle tri %d t %r, LBVH tri %d, brute force tri %d"
              % (k, rays[k, :3].tolist(), rays[k, 4:7].tolist(), int(wt[k]), float(want[k, 0]), int(got2["tri"][k]), int(got1["tri"][k])))
    assert_hits_equal(got2, want, name + " LBVH against the oracle")
    assert_hits_equal(got1, want, name + " brute force against the oracle")
    assert_hits_equal(got2, got1, name + " LBVH against brute force")
    assert np.array_equal(occ, (wt >= 0).astype(np.int32)) and np.array_equal(early, occ)


def words8(rays) -> np.ndarray:
    """pt_ray records (RAY_DTYPE or [N, 8] float32) as float32 [N, 8]"""
    return np.ascontiguousarray(np.asarray(rays)).view(np.float32).reshape(-1, 8)


def test_cluster_beside_an_outlier_needs_no_deep_stack(device):
    """slab541: 540 triangles in one cell of the 16-bit grid beside a triangle of 5e9, a box margin (PT_BVH_EPS x extent = 3e5) wider
    than the cluster, so that every ray that comes near enters every node.  A tallying render from the scene's camera reports the
    deepest traversal stack any ray needed: within the capacity of 64, and the render equals the oracle's -- no subtree was lost, no
    PT_ERR_TRAVERSAL was raised (the read and pt_sync would report it)."""
    import camera_oracle
    from conftest import assert_fb_equal
    from gpu_support import render

    tris, mats, _, cam = S.edge_scene("slab:15")[1]
    W, H, frames, depth = 24, 16, 2, 6
    want, st = camera_oracle.render(tris, mats, W, H, frames, cam, max_bounces=depth, want_stats=True)
    with options(device, ACCEL=2, BVH_TALLY=1):
        got, gst = render(device, tris, mats, W, H, frames, depth=depth, camera=cam, want_stats=True)
        assert shim.load().pt_sync(device._h) == shim.PT_OK
    stack = int(gst[shim.PT_STAT_BVH_MAX_STACK])
    print("slab541: deepest traversal stack %d of 64, %d nodes entered and %d triangles tested by %d rays"
          % (stack, int(gst[shim.PT_STAT_BVH_NODES]), int(gst[shim.PT_STAT_BVH_TRIS]), int(gst[shim.PT_STAT_RAYS])))
    assert 1 <= stack <= 64
    assert_fb_equal(got, want, "slab541, tallying render")
    assert int(gst[shim.PT_STAT_RAYS]) == st["rays"]


def test_snapshot_refuses_when_no_lbvh_stands(device):
    from oclpathtracer_amd.query import RayCaster

    lib = shim.load()
    tris = S.soup(700, 61)
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=1):
            rc.closest(_probe_rays())                           # the scene is prepared, no hierarchy is built
        info = shim.BvhInfo()
        assert lib.pt_bvh_snapshot(device._h, ctypes.byref(info), None, 0, None) == shim.PT_ERR_INVALID
        assert lib.pt_bvh_snapshot(device._h, None, None, 0, None) == shim.PT_ERR_INVALID
        with options(device, ACCEL=2):
            rc.closest(_probe_rays())
            assert lib.pt_bvh_snapshot(device._h, ctypes.byref(info), None, 0, None) == shim.PT_OK and info.records > 700
            small = np.zeros((8, 64), np.uint8)
            assert lib.pt_bvh_snapshot(device._h, ctypes.byref(info), small.ctypes.data_as(ctypes.c_void_p), 8, None) == shim.PT_ERR_RANGE
            assert not small.any()
    finally:
        rc.release()


def _built_scenes():
    from oclpathtracer_amd import scene

    yield "cornell", lambda: scene.load_model()[0]
    for n in (300, 2000, 20000, 200000):
        yield "soup%d" % n, (lambda n=n: scene.make_soup(n)[0])
    for kind in ("two", "three", "nine", "duplicates", "clustered", "many_big", "flat"):
        yield "edge_" + kind, (lambda kind=kind: S.bvh_edge(kind)[0])
    for delta in (0.3, 0.03, 0.003, 0.0003):
        yield "tiles%g" % delta, (lambda delta=delta: S.horizon_tiles(delta)[0])


@pytest.mark.parametrize("name", ["cornell", "soup300", "soup2000", "soup20000", "soup200000", "edge_two", "edge_three", "edge_nine",
                                  "edge_duplicates", "edge_clustered", "edge_many_big", "edge_flat", "tiles0.3", "tiles0.03", "tiles0.003",
                                  "tiles0.0003"])
def test_built_hierarchy_passes_the_checker(device, name):
    """one build each, no rays but the few that make the shim build"""
    from oclpathtracer_amd.query import RayCaster

    tris = dict(_built_scenes())[name]()
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=2):
            rc.closest(_probe_rays())
            out = check_hierarchy(device, tris, name)
    finally:
        rc.release()
    assert out["nodes"] >= 1          # (every triangle of the smallest scenes is big: a root without children)
