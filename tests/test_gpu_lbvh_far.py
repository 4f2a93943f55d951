"""Rays that start far outside the scene, through the LBVH and through the brute-force search, against the CPU oracle bit for bit.

The boxes of the LBVH are grown by a margin sized by the SCENE (PT_BVH_EPS x its largest |coordinate|); the displacement of a
binary32 hit grows with the distance the RAY has travelled.  tests/test_lbvh_margin_cpu.py measures, on the host, that from
D / m = 10^4 on (m: the scene's largest |coordinate|) the exact test accepts hits whose scene-margin box the ray does not touch;
the traversal therefore widens every slab by PT_BVH_RAY_EPS x the origin's largest |coordinate| (csrc/pt_bvh.hip).  Here every
family of tests/lbvh_far.py -- rays aimed at triangle edges at incidence cos 0.01 .. 1, rays parallel to an axis, rays with a +-0
component, rays whose tmax ends exactly at their hit -- runs at D / m = 1 .. 10^5 on both scenes under PT_OPT_ACCEL 1 and 2:
closest hits, the occlusion query and the early-exit occlusion search must equal the oracle's.

Oracle hit shares of the families (asserted >= 20 % below; measured on the host): tile scene edge 54-67 %, axis 46-56 %,
zero 54-67 %, tmax 50 %; soup edge 53-68 %, axis 61-67 %, zero 61-69 %, tmax 50 %.
"""
import numpy as np
import pytest

import ao_oracle
import camera_oracle
import lbvh_far as F
import query_oracle as qo
import scenes
from conftest import assert_fb_equal
from gpu_support import assert_hits_equal, options, render
from oclpathtracer_amd import shim

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name, dm):
    """(triangles, {family: rays}, {family: oracle records}) of a scene at a distance; the oracle runs once per case."""
    if (name, dm) not in _CASES:
        tris, fam = F.families(name, dm, qo.closest_threads)
        _CASES[(name, dm)] = (tris, fam, {k: qo.closest_threads(tris, r) for k, r in fam.items()})
    return _CASES[(name, dm)]


def _diagnose(rays, got_tri, want, dm, what, limit=6):
    """per-ray report of the first mismatches: the ray, the oracle's triangle and t, what the device found"""
    wt = want[:, 1].view(np.int32)
    bad = np.flatnonzero(got_tri != wt)
    if len(bad):
        print("%s at D/m = %g: %d of %d rays differ (device lost %d oracle hits)" % (what, dm, len(bad), len(rays), int((got_tri[bad] < 0).sum())))
    for k in bad[:limit]:
        print("  ray %d: origin %r tmax %r dir %r -> oracle tri %d t %r, device tri %d"
              % (k, rays[k, :3].tolist(), float(rays[k, 3]), rays[k, 4:7].tolist(), int(wt[k]), float(want[k, 0]), int(got_tri[k])))
    return len(bad)


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("dm", F.DISTANCES)
@pytest.mark.parametrize("name", sorted(F.SCENES))
def test_far_families_bit_exact(device, name, dm, accel):
    from oclpathtracer_amd.query import RayCaster

    tris, fam, wants = _case(name, dm)
    lib = shim.load()
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=accel):
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            for k in sorted(fam):
                rays, want = fam[k], wants[k]
                what = "%s/%s a%d" % (name, k, accel)
                assert len(rays) >= 100_000
                wt = want[:, 1].view(np.int32)
                share = float((wt >= 0).mean())
                print("%s at D/m = %g: the oracle hits with %.1f %% of %d rays" % (what, dm, 100 * share, len(rays)))
                assert share >= 0.2, "%s: a family that hardly hits tests nothing" % what
                got = rc.closest(rays)
                occ = rc.occluded(rays)
                early = rc.occluded(rays, early_exit=True)
                bad = _diagnose(rays, got["tri"], want, dm, what)
                for label, o in (("occluded", occ), ("pt_occluded_rays", early)):
                    _diagnose(rays, np.where(o != 0, np.where(wt >= 0, wt, 0x3fffffff), -1).astype(np.int32),
                              want, dm, "%s %s" % (what, label))   # (an occluded ray the oracle misses shows as triangle 2^30 - 1)
                assert bad == 0, "%s at D/m = %g: %d rays differ from the oracle" % (what, dm, bad)
                assert_hits_equal(got, want, what)
                assert np.array_equal(occ, (got["tri"] >= 0).astype(np.int32)), what + ": occluded != (tri >= 0)"
                assert np.array_equal(early, (got["tri"] >= 0).astype(np.int32)), what + ": pt_occluded_rays != (tri >= 0)"
            moved = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) - builds
            assert moved == (1 if accel == 2 else 0), "%s: the search that ran is not the one asked for" % what
    finally:
        rc.release()


def test_accel_auto_takes_the_lbvh_for_the_tile_scene(device):
    """576 triangles: PT_OPT_ACCEL = 0 walks the hierarchy too, and the farthest family stays exact"""
    from oclpathtracer_amd.query import RayCaster

    tris, fam, wants = _case("tile", 1e5)
    assert len(tris) >= 512
    lib = shim.load()
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=0):
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            got = rc.closest(fam["edge"])
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds + 1
    finally:
        rc.release()
    assert _diagnose(fam["edge"], got["tri"], wants["edge"], 1e5, "tile/edge a0") == 0
    assert_hits_equal(got, wants["edge"], "tile/edge a0")


def _far_view():
    """The tile scene with the soup above and below it, its materials, and a camera 10^4 scene sizes away (the scene is 6
    across) whose narrow field of view frames it."""
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.camera import Camera

    tris = np.concatenate([scenes.tile_scene(), scenes.soup(2000, 5)])
    mats = np.zeros(7, scene.MATERIAL_DTYPE)
    rng = np.random.default_rng(2)
    for m in range(7):
        mats[m]["albedo"] = tuple(rng.uniform(0.15, 0.95, 3)) + (1.0,)
        mats[m]["emissive"] = (20.0, 20.0, 20.0, 1.0) if m == 6 else (0.0, 0.0, 0.0, 1.0)
        mats[m]["type"] = scene.SPECULAR if m == 0 else scene.DIFFUSE
        mats[m]["roughness"] = np.float32(0.05) if m == 0 else 0.0
    # The eye stands ON the y axis: the reference's generateRay aims each primary ray at eye + 4 dir, which is rounded to the eye's
    # ulp; with one large coordinate only, the other two components of the direction keep their precision and the pixels still
    # resolve the scene (from a general position at this distance the image degenerates to a handful of directions).
    dist = 6.0e4
    fov = float(np.degrees(2 * np.arctan(4.5 / dist)))
    return tris, mats, Camera(eye=(0.0, dist, 0.0), center=(0.0, 0.37, 0.0), up=(0.0, 0.0, -1.0), fov_y_deg=fov)


def test_render_from_a_far_camera(device):
    tris, mats, cam = _far_view()
    W, H, frames = 96, 96, 3
    want, st = camera_oracle.render(tris, mats, W, H, frames, cam, want_stats=True)
    print("far camera: the oracle accepted %d hits over %d samples" % (st["accept"], W * H * frames))
    assert st["accept"] > 0.2 * W * H * frames, "the camera must frame the scene"
    got = {}
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            got[accel] = render(device, tris, mats, W, H, frames, camera=cam)
    assert_fb_equal(got[2], want, "far camera, LBVH against the oracle")
    assert_fb_equal(got[1], want, "far camera, brute force against the oracle")
    assert_fb_equal(got[2], got[1], "far camera, LBVH against brute force")


def test_ambient_occlusion_from_a_far_camera(device):
    from oclpathtracer_amd.ao import AORenderer

    tris, _, cam = _far_view()
    W, H, frames, K, radius = 64, 64, 2, 8, 1.5
    want = ao_oracle.counts(tris, W, H, 0, frames, K, radius, cam=cam)
    assert want[..., 1].sum() > 0.2 * W * H * frames and (want[..., 0] < K * want[..., 1]).any(), "hits, and some of them occluded"
    with options(device, ACCEL=2):
        r = AORenderer(device, tris, W, H, rays_per_sample=K, radius=radius, camera=cam, stripe_rows=1)
        try:
            r.render(frames, 0)
            got = r.read_counts()
        finally:
            r.release()
    assert np.array_equal(got, want), "far camera AO: counts differ at %d pixels" % int((got != want).any(-1).sum())
