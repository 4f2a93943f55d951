"""The look-at camera on the GPU: every render against the camera oracle (tests/camera_oracle.c), bit for bit, in every search
mode -- brute force with and without primary-ray masks, the tiled kernel, the LBVH -- with checkpointed chunks, image
stripes, camera changes in flight, rejected cameras and the drivers' set_camera."""
import ctypes
import math
import os
import time

import numpy as np
import pytest

import camera_oracle
from conftest import GOLDEN, assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import shim
from scenes import nested_boxes

pytestmark = pytest.mark.gpu

W, H, FRAMES = 64, 48, 4
CAMERAS = ["translated", "yawed30", "rolled", "fov20", "fov120", "inside_up", "far"]


def _cams():
    from oclpathtracer_amd.camera import Camera

    eye = (0.0, 2.75, 4.0)
    a = math.radians(30.0)
    r = math.radians(20.0)
    return {
        "translated": Camera((0.6, 2.2, 3.0), (0.6, 2.2, 2.0)),
        "yawed30": Camera(eye, (eye[0] - math.sin(a), eye[1], eye[2] - math.cos(a))),
        "rolled": Camera(eye, (0.0, 2.75, 3.0), up=(math.sin(r), math.cos(r), 0.0)),
        "fov20": Camera(eye, (0.0, 2.75, 3.0), fov_y_deg=20.0),
        "fov120": Camera(eye, (0.0, 2.75, 3.0), fov_y_deg=120.0),
        "inside_up": Camera((0.3, 1.5, -2.5), (0.0, 5.4, -2.8), up=(0.0, 0.0, -1.0)),
        "far": Camera((0.0, 2.75, 54.0), (0.0, 2.75, -2.8), fov_y_deg=20.0),
    }


MODES = {"brute_masks": dict(ACCEL=1, PRIMARY_MASKS=1), "brute_nomasks": dict(ACCEL=1, PRIMARY_MASKS=0), "lbvh": dict(ACCEL=2)}


def test_explicit_reference_camera_is_the_default(device, cornell):
    """pt_camera_reference() renders exactly what cam = NULL renders -- the golden image -- in every search mode."""
    from oclpathtracer_amd.camera import Camera

    tris, mats = cornell
    want = np.load(os.path.join(GOLDEN, "cornell_64x64_f8_d16.npy"))
    for name, opts in MODES.items():
        with options(device, **opts):
            none = render(device, tris, mats, 64, 64, 8)
            ref = render(device, tris, mats, 64, 64, 8, camera=Camera.reference())
        assert_fb_equal(none, want, "cam=NULL, %s" % name)
        assert_fb_equal(ref, want, "reference camera, %s" % name)


_ORACLE = {}


def _want(tris, mats, name, cam, depth, w=W, h=H, frames=FRAMES):
    key = (name, depth, w, h, frames, len(tris))
    if key not in _ORACLE:
        _ORACLE[key] = camera_oracle.render(tris, mats, w, h, frames, cam, max_bounces=depth, want_stats=True)
    return _ORACLE[key]


@pytest.mark.parametrize("depth", [16, 2])
@pytest.mark.parametrize("name", CAMERAS)
def test_moved_cameras_match_the_camera_oracle(device, cornell, name, depth):
    tris, mats = cornell
    assert list(_cams()) == CAMERAS, "CAMERAS must name every camera of _cams(), in its order"
    cam = _cams()[name]
    want, st = _want(tris, mats, name, cam, depth)
    for mode, opts in MODES.items():
        with options(device, **opts):
            got, gst = render(device, tris, mats, W, H, FRAMES, camera=cam, depth=depth, want_stats=True)
        assert_fb_equal(got, want, "%s, depth %d, %s" % (name, depth, mode))
        assert int(gst[0]) == W * H * FRAMES
        assert int(gst[1]) == st["rays"], (name, depth, mode)


def test_tiled_kernel_with_a_moved_camera(device, cornell):
    """257 ... 511 triangles: the brute-force search with LDS record tiles, seen from a moved camera."""
    big, mats = nested_boxes(8)
    assert 256 < len(big) < 512
    cam = _cams()["yawed30"]
    want, st = camera_oracle.render(big, mats, W, H, 3, cam, want_stats=True)
    with options(device, ACCEL=1):
        got, gst = render(device, big, mats, W, H, 3, camera=cam, want_stats=True)
    assert_fb_equal(got, want, "tiled brute force, moved camera")
    assert int(gst[1]) == st["rays"]


@pytest.mark.parametrize("kernel", ["table", "lbvh"])
def test_checkpointed_chunks_under_a_moved_camera(device, cornell, kernel):
    """PT_OPT_CHUNK_FRAMES 3, 8 frames: three checkpointed launches and a draining one carry paths across launch boundaries
    under a moved camera -- the table kernel on the Cornell box, the LBVH kernel on a soup framed by Camera.fit."""
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.camera import Camera

    if kernel == "table":
        tris, mats = cornell
        cam, opts = _cams()["translated"], dict(ACCEL=1)
    else:
        tris, mats = scene.make_soup(2000)
        cam, opts = Camera.fit(tris, view_dir=(0.4, -0.3, -1.0), aspect=W / H), dict(ACCEL=0)
    want, st = camera_oracle.render(tris, mats, W, H, 8, cam, want_stats=True)
    with options(device, CHUNK_FRAMES=3, **opts):
        got, gst = render(device, tris, mats, W, H, 8, camera=cam, want_stats=True)
    assert_fb_equal(got, want, "checkpointed chunks, %s kernel, moved camera" % kernel)
    assert int(gst[shim.PT_STAT_RAYS]) == st["rays"]
    assert int(gst[shim.PT_STAT_CARRIED]) > 0


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_stripes_reassemble_to_the_one_device_image(device, cornell, n_ranks):
    """Seeds and camera rays use GLOBAL pixel ids: the ranks' stripes, rendered here one after another on the one GPU and put
    back in their rows, are the one-device image for a moved camera."""
    tris, mats = cornell
    cam = _cams()["rolled"]
    w, h, frames, stripe = 64, 50, 3, 4
    one = render(device, tris, mats, w, h, frames, camera=cam)
    want = camera_oracle.render(tris, mats, w, h, frames, cam)
    assert_fb_equal(one, want, "one device")
    img = np.full((h, w, 4), np.nan, np.float32)
    from oclpathtracer_amd.render import Renderer

    for rank in range(n_ranks):
        r = Renderer(device, tris, mats, w, h, n_ranks=n_ranks, rank=rank, stripe_rows=stripe, camera=cam)
        try:
            r.render(frames)
            img[r.global_rows()] = r.read().reshape(-1, w, 4)
        finally:
            r.release()
    assert_fb_equal(img.reshape(-1, 4), one, "%d ranks reassembled" % n_ranks)


@pytest.mark.parametrize("accel", [1, 2])
def test_camera_changes_in_flight(device, cornell, accel):
    """A, B, A, B into four framebuffers with no wait in between, then A continues the first one's accumulation: every image
    is the oracle's, the LBVH is not rebuilt, the workspace does not grow, and the calls return long before the GPU is done."""
    from oclpathtracer_amd import adl
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    lib = shim.load()
    A, B = _cams()["yawed30"], _cams()["far"]
    w = h = 512
    F = 32
    wantA = camera_oracle.render(tris, mats, w, h, F, A)
    wantB = camera_oracle.render(tris, mats, w, h, F, B)
    wantA2 = camera_oracle.render(tris, mats, w, h, F, A, frame_begin=F, fb=wantA.copy())
    with options(device, ACCEL=accel):
        r = Renderer(device, tris, mats, w, h, camera=A)
        fbs = [r.fb] + [adl.Buffer(device, w * h, adl.float4) for _ in range(3)]
        try:
            r.render(F, frame_begin=0)                      # warm: scene, LBVH, masks, ring
            device.waitForCompletion()
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            ws = lib.pt_device_workspace_memory(device._h)
            t0 = time.perf_counter()
            for k, cam in enumerate((A, B, A, B)):
                r.set_camera(cam)
                r.render(F, frame_begin=0, fb=fbs[k])
            r.set_camera(A)
            r.render(F, frame_begin=F, fb=fbs[0])
            t_enqueue = time.perf_counter() - t0
            device.waitForCompletion()
            t_total = time.perf_counter() - t0
            for k, want in enumerate((wantA2, wantB, wantA, wantB)):
                got = np.empty((w * h, 4), np.float32)
                fbs[k].read(got, w * h)
                device.waitForCompletion()
                assert_fb_equal(got, want, "framebuffer %d, accel %d" % (k, accel))
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds
            assert lib.pt_device_workspace_memory(device._h) == ws
        finally:
            for b in fbs[1:]:
                b.release()
            r.release()
    print("5 renders with 4 camera changes: enqueued in %.2f ms, finished after %.2f ms" % (t_enqueue * 1e3, t_total * 1e3))
    assert t_enqueue < 0.5 * t_total


def test_invalid_camera_is_refused_and_renders_nothing(device, cornell):
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    lib = shim.load()
    r = Renderer(device, tris, mats, W, H)
    try:
        sentinel = np.full((W * H, 4), 0.25, np.float32)
        r.fb.write(sentinel, W * H)
        p = shim.RenderParams()
        p.width, p.height, p.frame_begin, p.frame_count, p.max_bounces = W, H, 0, 2, 16
        p.num_triangles, p.num_materials, p.stripe_rows, p.n_ranks, p.rank = len(tris), len(mats), 16, 1, 0
        for bad in (dict(center=(0.0, 2.75, 4.0)), dict(up=(0.0, 0.0, 1.0), center=(0.0, 2.75, 5.0)), dict(fov=180.0),
                    dict(fov=float("nan")), dict(reserved=1)):
            c = shim.Camera()
            lib.pt_camera_reference(ctypes.byref(c))
            if "center" in bad:
                c.center[:] = bad["center"]
            if "up" in bad:
                c.up[:] = bad["up"]
            if "fov" in bad:
                c.fov_y_deg = bad["fov"]
            if "reserved" in bad:
                c.reserved[5] = 1
            rc = lib.pt_render_frames_camera(device._h, r.tbuf._h, r.mbuf._h, r.fb._h, ctypes.byref(p), ctypes.byref(c), None, None)
            assert rc == shim.PT_ERR_INVALID, bad
        assert_fb_equal(r.read(), sentinel, "framebuffer after refused renders")
    finally:
        r.release()


def test_set_camera_restarts_accumulation(device, cornell):
    from oclpathtracer_amd.progressive import ProgressiveRenderer
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    A, B = _cams()["translated"], _cams()["inside_up"]
    wantB = camera_oracle.render(tris, mats, W, H, 5, B)
    r = Renderer(device, tris, mats, W, H, camera=A)
    try:
        r.render(3)
        r.render(2)
        assert r.frames_done == 5
        r.set_camera(B)
        assert r.frames_done == 0 and r.camera == B
        r.render(2)
        r.render(3)
        assert_fb_equal(r.read(), wantB, "Renderer after set_camera")
    finally:
        r.release()
    p = ProgressiveRenderer(device, tris, mats, W, H, frames_per_step=2, camera=A)
    try:
        p.step()
        p.step(3)
        p.set_camera(B)
        assert p.frames_done == 0
        p.step(3)
        p.step(2)
        frames, img = p.latest(block=True)
        assert frames == 5
        assert_fb_equal(np.array(img, copy=True), wantB, "ProgressiveRenderer after set_camera")
    finally:
        p.release()
