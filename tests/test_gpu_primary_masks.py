"""The primary rays' candidate masks (pt_primary_mask_kernel) against the reference's own test, through the C ABI: the table the
trace kernel reads (pt_primary_mask_snapshot) keeps every triangle the reference ACCEPTS for any sample of the pixel (the
restatement tests/primary_accept.c says which), the images stay the oracle's, the masks are really stronger than the cull and the
u strip alone, and a camera change remakes them in place."""
import ctypes

import numpy as np
import pytest

import camera_oracle
import primary_accept
from conftest import assert_fb_equal
from oclpathtracer_amd import scene as _scene, shim
from oclpathtracer_amd.camera import Camera
from oclpathtracer_amd.render import Renderer

pytestmark = pytest.mark.gpu

FRAMES = 32          # the superset is checked over frames 0 .. 31
RENDER_FRAMES = 2
EYE, CENTER = (0.0, 2.75, 4.0), (0.0, 2.75, 3.0)   # the reference camera's (GenerateColors.cl:263-264)


def snapshot(device, expect_pixels):
    lib = shim.load()
    n = ctypes.c_uint32(0)
    shim.check(lib.pt_primary_mask_snapshot(device._h, ctypes.byref(n), None, 0))
    assert n.value == expect_pixels, "the table stands for %d pixels, the render has %d" % (n.value, expect_pixels)
    out = np.zeros((max(n.value, 1), 2), np.uint32)
    shim.check(lib.pt_primary_mask_snapshot(device._h, ctypes.byref(n), out.ctypes.data_as(ctypes.c_void_p), len(out)))
    return out[: n.value]


def quad(a, b, c, d, mat=0):
    """(a,b,c),(c,d,a)"""
    t = np.zeros(2, _scene.TRIANGLE_DTYPE)
    for k, (p1, p2, p3) in enumerate(((a, b, c), (c, d, a))):
        t["p1"][k, :3], t["p2"][k, :3], t["p3"][k, :3] = p1, p2, p3
        t["id"][k] = mat
    return t


def quads_64():
    """64 triangles: the box and the first 14 quads of a shrunk copy of itself inside it -- both chunk words are in use"""
    tris, mats = _scene.load_model()
    inner = tris[:28].copy()
    for f in ("p1", "p2", "p3"):
        inner[f][:, :3] = inner[f][:, :3] * np.float32(0.4) + np.array([0.3, 1.2, -1.9], np.float32)
    out = np.concatenate([inner, tris])     # (the inner copy first: nothing of it is hidden behind an earlier, closer hit)
    assert len(out) == 64
    return out, mats


def edge_quads():
    """Four quads in FRONT of the box in the triangle order (an accepted hit of theirs is not pre-empted by a closer one found
    earlier), seen from the reference camera at an odd height, where the centre row's rays are exactly horizontal at the pixel's centre:
      0, 1  in the plane y = eye.y: the plane contains the eye, e2 . qvec is 0
      2, 3  wholly behind the eye, turned so that the cull test passes: u and v pass for some rays, t < 0 for all
      4, 5  horizontal, 0.25 below the eye, 8 to 20 away: det is 0 at the centre of the centre row's pixels, positive in the
            lower half of their footprint, whose rays hit it
      6, 7  without area (b = a, d = c)"""
    tris, mats = _scene.load_model()
    y = 2.75
    in_plane = quad((-0.5, y, 2.0), (-0.5, y, 1.0), (0.5, y, 1.0), (0.5, y, 2.0))
    behind = quad((-1.0, 1.75, 6.0), (1.0, 1.75, 6.0), (1.0, 3.75, 6.0), (-1.0, 3.75, 6.0))   # cross(e2, e1) points along -z
    yl = 2.5
    level = quad((-1.0, yl, -16.0), (-1.0, yl, -4.0), (1.0, yl, -4.0), (1.0, yl, -16.0))   # cross(e2, e1) points down
    flat = quad((-0.2, 2.0, 1.0), (-0.2, 2.0, 1.0), (0.3, 3.0, 1.0), (0.3, 3.0, 1.0))
    return np.concatenate([in_plane, behind, level, flat, tris]), mats


def _cornell():
    return _scene.load_model()


def cam(**kw):
    kw.setdefault("eye", EYE)
    kw.setdefault("center", CENTER)
    return Camera(kw.pop("eye"), kw.pop("center"), **kw)


# name: (scene, W, H, camera or None, Renderer keywords)
CASES = {
    "cornell_64x64": (_cornell, 64, 64, None, {}),
    "cornell_33x17": (_cornell, 33, 17, None, {}),
    "cornell_1x1": (_cornell, 1, 1, None, {}),
    "cornell_2x3": (_cornell, 2, 3, None, {}),
    "fov_1": (_cornell, 24, 24, cam(fov_y_deg=1.0), {}),
    "fov_179": (_cornell, 24, 24, cam(fov_y_deg=179.0), {}),
    "cornell_96x16": (_cornell, 96, 16, None, {}),
    # the moved cameras of tools/camera_rates.py
    "yawed30": (_cornell, 40, 24, Camera((0.0, 2.75, 4.0), (-0.5, 2.75, 4.0 - 0.8660254)), {}),
    "inside_up": (_cornell, 40, 24, Camera((0.3, 1.5, -2.5), (0.0, 5.4, -2.8), up=(0.0, 0.0, -1.0)), {}),
    "far_fov20": (_cornell, 40, 24, Camera((0.0, 2.75, 54.0), (0.0, 2.75, -2.8), fov_y_deg=20.0), {}),
    "rank1_of_3": (_cornell, 20, 30, None, dict(n_ranks=3, rank=1, stripe_rows=4)),
    "quads_64": (quads_64, 48, 48, None, {}),
    "edge_quads": (edge_quads, 33, 17, None, {}),
}


def oracle_image(oracle, tris, mats, W, H, frames, camera, rows):
    """the local rows of the oracle's image and its ray count over them"""
    fb = np.zeros((H * W, 4), np.float32)
    rays = 0
    runs = np.split(rows, np.flatnonzero(np.diff(rows) != 1) + 1) if len(rows) else []
    for run in runs:
        kw = dict(fb=fb, gid_begin=int(run[0]) * W, gid_count=len(run) * W, want_stats=True)
        if camera is None:
            _, st = oracle.render(tris, mats, W, H, frames, **kw)
        else:
            _, st = camera_oracle.render(tris, mats, W, H, frames, camera, **kw)
        rays += st["rays"]
    gids = (rows[:, None] * W + np.arange(W)[None, :]).reshape(-1)
    return fb[gids], rays, gids


@pytest.mark.parametrize("name", list(CASES))
def test_masks_keep_what_the_reference_accepts(device, oracle, name):
    """Superset: per pixel, the union over frames 0..31 of the accepted sets lies inside the mask.  Image parity: the render that
    made the masks gives the oracle's pixels and ray count, bit for bit."""
    make, W, H, camera, kw = CASES[name]
    tris, mats = make()
    r = Renderer(device, tris, mats, W, H, camera=camera, want_stats=True, **kw)
    try:
        r.render(RENDER_FRAMES)
        got = r.read()
        rays = int(r.read_stats_raw()[shim.PT_STAT_RAYS])
        snap = snapshot(device, r.local_pixels)
        rows = r.global_rows()
    finally:
        r.release()
    want, want_rays, gids = oracle_image(oracle, tris, mats, W, H, RENDER_FRAMES, camera, rows)
    assert_fb_equal(got, want, name)
    assert rays == want_rays, "%s: %d rays, the oracle traced %d" % (name, rays, want_rays)

    acc, reach, _, _ = primary_accept.union(tris, W, H, FRAMES, cam=camera, gid=gids)
    mask = primary_accept.mask_bits(snap, len(tris))
    lost = acc & ~mask
    assert not lost.any(), "%s: %d pixels lost an accepted triangle (first: local pixel %d, triangles %#x)" % (
        name, int((lost != 0).sum()), int(np.flatnonzero(lost)[0]), int(lost[np.flatnonzero(lost)[0]]))
    if len(tris) < 64:
        assert not (mask >> np.uint64(len(tris))).any(), "%s: bits above the triangle count" % name
    print("%s: mean popcount %.3f; accepted union %.3f, cull-and-u union %.3f" % (
        name, primary_accept.popcount(mask).mean(), primary_accept.popcount(acc).mean(), primary_accept.popcount(reach).mean()))
    if name == "edge_quads":
        assert not (mask & np.uint64(0b11001111)).any(), "a quad through the eye, behind it or without area was kept"
        assert (acc & np.uint64(0b110000)).any(), "no ray of the restatement hits the level quad: the case is empty"
        centre = slice(8 * W, 9 * W)   # d.y = 0 at these pixels' centres
        assert (acc[centre] & np.uint64(0b110000)).any(), "the level quad is not hit from the centre row"


def test_masks_are_stronger_than_cull_and_u(device, cornell):
    """Cornell box, reference camera, 256 x 256: L = the mean size of the union over 32 frames of the accepted sets, P = the same
    for the cull-and-u sets (both from the restatement alone).  L <= mean popcount <= (L + P) / 2: masks that only restate pass 1
    sit at P or above."""
    tris, mats = cornell
    W = H = 256
    r = Renderer(device, tris, mats, W, H)
    try:
        r.render(1, max_bounces=1)
        snap = snapshot(device, W * H)
    finally:
        r.release()
    acc, reach, _, _ = primary_accept.union(tris, W, H, FRAMES)
    mask = primary_accept.mask_bits(snap, len(tris))
    L, P = primary_accept.popcount(acc).mean(), primary_accept.popcount(reach).mean()
    pop = primary_accept.popcount(mask).mean()
    print("accepted union L = %.4f, mean popcount = %.4f, cull-and-u union P = %.4f" % (L, pop, P))
    assert not (acc & ~mask).any()
    assert L <= pop <= (L + P) / 2


def test_camera_change_remakes_the_masks_in_place(device, cornell):
    """Two renders on one handle with the camera changed in between: other masks, the same workspace, no LBVH build."""
    tris, mats = cornell
    lib = shim.load()
    W, H = 64, 48
    r = Renderer(device, tris, mats, W, H)
    try:
        r.render(1)
        first = snapshot(device, W * H).copy()
        builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
        ws = lib.pt_device_workspace_memory(device._h)
        r.set_camera(Camera((0.0, 2.75, 4.0), (-0.5, 2.75, 4.0 - 0.8660254)))
        r.render(1)
        second = snapshot(device, W * H)
        assert not np.array_equal(first, second), "the masks did not follow the camera"
        assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds
        assert lib.pt_device_workspace_memory(device._h) == ws
        r.set_camera(None)
        r.render(1)
        assert np.array_equal(snapshot(device, W * H), first), "back at the first camera, other masks"
    finally:
        r.release()
