"""Indirect illumination (pt_render_indirect) on the MI355X, bit for bit.

The framebuffer -- and where the workspace holds every frame, the radiance before the fold -- is compared with
tests/indirect_oracle.c, which composes the estimator from the CPU oracle's own steps.  Two identities need no restatement: with no
lights the image is the fused renderer's at the same depth (the second statement of the bounce against pt_shade), at one bounce
it is DirectRenderer's."""
import ctypes
from functools import partial

import numpy as np
import pytest

import indirect_edges as ie
import indirect_oracle as io
from conftest import assert_fb_equal
from gpu_support import (SEARCHES, LitBuffers, assert_cut_short_search_is_reported, assert_lit_argument_errors, harness_ppm,
                         lit_with_samples, options, render)
from indirect_scenes import lbvh_boxes, tiled_boxes
from oclpathtracer_amd import shim
from scenes import GLOSSY_SHIFTS, glossy_room

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int32)
W, H = 40, 24
CASES = ((16, 1), (3, 4))   # (B, K)
FRAMES = 4

_Buffers = partial(LitBuffers, "pt_render_indirect")


def _indirect(device, tris, mats, W, H, frames, K, B, want_samples=False, lights=None, camera=None, **kw):
    fb, ws = lit_with_samples(device, (tris, mats, lights, camera), W, H, frames, K, max_bounces=B, **kw)
    return (fb, ws[:frames].reshape(-1, 3)) if want_samples else fb


def _want(name, frames, K, B):
    """the restatement's framebuffer and its radiance before the fold, frame-major as the workspace holds it, of a scene of
    scenes.edge_scene: computed once, shared, never written to"""
    return ie.wanted(name, W, H, frames, K, B)


@pytest.fixture(scope="module")
def cornell_want():
    return {(B, K): _want("cornell", FRAMES, K, B) for B, K in CASES}


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_bit_exact_against_the_restatement(device, cornell, cornell_want, quad, accel):
    """brute force with the LDS table and the LBVH forced on the 36-triangle scene, under every filter"""
    tris, mats = cornell
    for (B, K), (want_fb, want_rad) in cornell_want.items():
        what = "B%d K%d q%d a%d" % (B, K, quad, accel)
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            fb, rad = _indirect(device, tris, mats, W, H, FRAMES, K, B, want_samples=True, chunk_frames=FRAMES)
            chunked = _indirect(device, tris, mats, W, H, FRAMES, K, B, chunk_frames=3)   # 3 + 1 frames: two launches, two folds
        assert_fb_equal(rad, want_rad, what + ": radiance before the fold")
        assert_fb_equal(fb, want_fb, what)
        assert_fb_equal(chunked, want_fb, what + " in two chunks")


def test_tiled_brute_force(device):
    tris, mats = tiled_boxes()
    want_fb, want_rad = _want("nested:10", 2, 2, 4)
    with options(device, ACCEL=1):
        fb, rad = _indirect(device, tris, mats, W, H, 2, 2, 4, want_samples=True)
    assert_fb_equal(rad, want_rad, "tiled brute force: radiance before the fold")
    assert_fb_equal(fb, want_fb, "tiled brute force")


@pytest.mark.parametrize("B", [2, 16])
def test_no_lights_is_the_renderer(device, cornell, B):
    tris, mats = cornell
    want = render(device, tris, mats, W, H, 3, depth=B, stripe_rows=1)
    got = _indirect(device, tris, mats, W, H, 3, 4, B, lights=NONE, chunk_frames=2)
    assert_fb_equal(got, want, "no lights against Renderer.render(max_bounces=%d)" % B)


@pytest.mark.parametrize("K", [1, 4])
def test_one_bounce_is_direct_illumination(device, cornell, K):
    from oclpathtracer_amd.direct import DirectRenderer

    tris, mats = cornell
    d = DirectRenderer(device, tris, mats, W, H, light_samples=K, stripe_rows=1)
    try:
        d.render(3)
        want = d.read()
    finally:
        d.release()
    assert_fb_equal(_indirect(device, tris, mats, W, H, 3, K, 1), want, "B = 1 against DirectRenderer, K = %d" % K)


@pytest.fixture(scope="module")
def lbvh_scene():
    return lbvh_boxes()


def test_lbvh_against_the_restatement_and_brute_force(device, lbvh_scene):
    tris, mats = lbvh_scene
    want_fb, want_rad = _want("nested:15", 2, 2, 4)
    res = {}
    for accel in (0, 2, 1):
        with options(device, ACCEL=accel):
            res[accel] = _indirect(device, tris, mats, W, H, 2, 2, 4, want_samples=True)
    assert_fb_equal(res[0][1], want_rad, "LBVH (automatic): radiance before the fold")
    assert_fb_equal(res[0][0], want_fb, "LBVH (automatic) against the restatement")
    assert_fb_equal(res[2][0], want_fb, "LBVH (forced) against the restatement")
    assert_fb_equal(res[1][0], res[2][0], "forced brute force against the LBVH")
    gid, frame = io.all_samples(W, H, 2)
    _, vertices, end, later = io.samples(tris, mats, W, H, gid, frame, 2, 4)
    assert vertices.max() == 4 and later[:, 0].sum() > 0 and later[:, 1].sum() > 0 and (end == io.END_MISS).any()


def test_lbvh_refill_over_more_samples_than_the_grid(device, lbvh_scene):
    """More samples than the persistent grid holds lanes (at most five workgroups of 256 per CU, the driver's other kernels' figure;
    this kernel runs fewer), so lanes whose path has ended take further samples while their neighbours are in mid-path.  An error
    common to the LBVH and brute force passes their comparison, so every 7th sample and every sample past the grid's lanes is also
    compared with the restatement, before the fold; at K = 2 a refilled lane's path has light samples that cast no ray between
    those that do."""
    tris, mats = lbvh_scene
    lanes = shim.load().pt_device_num_cus(device._h) * 5 * 256
    Wb = 768
    Hb = lanes // Wb + 64
    assert Wb * Hb > lanes
    gid = np.arange(Wb * Hb)
    gid = gid[(gid % 7 == 0) | (gid >= lanes)]
    for K in (1, 2):
        res = {}
        for accel in (2, 1):
            with options(device, ACCEL=accel):
                res[accel] = _indirect(device, tris, mats, Wb, Hb, 1, K, 3, chunk_frames=1, want_samples=True)
        assert_fb_equal(res[2][0], res[1][0], "refill, K %d: LBVH against brute force" % K)
        want = io.samples(tris, mats, Wb, Hb, gid, np.zeros(len(gid), np.int32), K, 3)[0]
        for accel in (2, 1):
            assert_fb_equal(res[accel][1][gid], want, "refill, K %d, accel %d: radiance before the fold" % (K, accel))


@pytest.mark.parametrize("shift", GLOSSY_SHIFTS)
def test_glossy_room(device, shift):
    """the BRDF step's guarded quotients at every roughness edge, feeding light samples at later vertices"""
    tris, mats = glossy_room(shift)
    want_fb, want_rad = _want("glossy:%d" % shift, 3, 1, 4)
    fb, rad = _indirect(device, tris, mats, W, H, 3, 1, 4, want_samples=True)
    assert_fb_equal(rad, want_rad, "glossy room %d: radiance before the fold" % shift)
    assert_fb_equal(fb, want_fb, "glossy room %d" % shift)


def test_progressive_frame_zero_cameras_and_a_rejected_camera(device, cornell):
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = cornell
    B, K = 4, 2
    want = io.render(tris, mats, W, H, 0, 5, K, B)
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, stripe_rows=1, chunk_frames=2)
    try:
        r.fb.write(np.full((W * H, 4), np.nan, np.float32), W * H)
        r.render(2)                       # frame 0: whatever the buffer held is overwritten
        r.render(3)                       # continues at frame 2: 2 + 1 frames
        assert r.frames_done == 5
        assert_fb_equal(r.read(), want, "progressive")
        r.render(5, 0)
        assert_fb_equal(r.read(), want, "one call, frame_begin 0 over a dirty framebuffer")
    finally:
        r.release()
    cam = Camera(eye=(-2.0, 1.0, 3.0), center=(1.0, 3.0, -2.0), up=(0.1, 1.0, 0.0), fov_y_deg=75.0)
    assert_fb_equal(_indirect(device, tris, mats, W, H, 2, K, B, camera=cam), io.render(tris, mats, W, H, 0, 2, K, B, cam=cam), "camera")
    b = _Buffers(device, tris, mats, W, H)
    try:
        bad = shim.Camera()
        b.lib.pt_camera_reference(ctypes.byref(bad))
        bad.center[:] = bad.eye[:]
        assert b.call(b.params(2), cam=ctypes.byref(bad)) == shim.PT_ERR_INVALID
        b.assert_untouched()
    finally:
        b.release()


def test_stripes_equal_the_single_rank_rows(device, cornell):
    tris, mats = cornell
    S, R = 4, 3
    full = _indirect(device, tris, mats, W, H, 2, 1, 4, stripe_rows=S).reshape(H, W, 4)
    for k in range(R):
        rows = (np.arange(H) // S) % R == k
        got = _indirect(device, tris, mats, W, H, 2, 1, 4, stripe_rows=S, n_ranks=R, rank=k)
        assert_fb_equal(got, full[rows], "rank %d of %d" % (k, R))


def test_chunks_do_not_change_the_image(device, cornell):
    tris, mats = cornell
    one = _indirect(device, tris, mats, W, H, 5, 1, 4, chunk_frames=1)
    all_ = _indirect(device, tris, mats, W, H, 5, 1, 4, chunk_frames=5)
    assert_fb_equal(one, all_, "a workspace of one frame against one of all five")


def test_interleaved_with_renders_direct_and_ao(device, cornell, oracle):
    import ao_oracle
    import direct_oracle as do
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    Wi = Hi = 32
    lib = shim.load()
    with options(device, ACCEL=2, CHUNK_FRAMES=3):
        r = Renderer(device, tris, mats, Wi, Hi, want_stats=True, stripe_rows=1)
        a = r.ao_renderer(rays_per_sample=4, radius=0.9)
        dr = r.direct_renderer(light_samples=2, chunk_frames=2)
        ir = r.indirect_renderer(light_samples=1, max_bounces=4, chunk_frames=2)
        try:
            assert ir.lights.tolist() == [10, 11] and ir.max_bounces == 4
            r.render(4)
            ir.render(3)
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            ws = device.getWorkspaceMemory()
            dr.render(3)
            a.render(2)
            r.render(3)
            ir.render(2)
            dr.render(2)
            a.render(2)
            assert_fb_equal(r.read(), oracle.render(tris, mats, Wi, Hi, 7), "render around the others")
            assert_fb_equal(ir.read(), io.render(tris, mats, Wi, Hi, 0, 5, 1, 4), "indirect around the others")
            assert_fb_equal(dr.read(), do.render(tris, mats, Wi, Hi, 0, 5, 2), "direct around the others")
            assert np.array_equal(a.read_counts(), ao_oracle.counts(tris, Wi, Hi, 0, 4, 4, 0.9))
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds
            assert device.getWorkspaceMemory() == ws
        finally:
            ir.release()
            dr.release()
            a.release()
            r.release()


# ---- the raw C ABI ------------------------------------------------------------------------------------------------------------
def test_c_abi_argument_errors_leave_the_framebuffer_untouched(device, cornell):
    tris, mats = cornell
    E_INV = shim.PT_ERR_INVALID
    b = _Buffers(device, tris, mats, 16, 8)
    try:
        for kw in [dict(max_bounces=0), dict(max_bounces=65536), dict(max_bounces=-1)] + [dict(reserved=k) for k in range(4)]:
            assert b.call(b.params(2, **kw)) == E_INV, kw
        assert_lit_argument_errors(b)
        for ok in (dict(max_bounces=1), dict(max_bounces=65535, num_triangles=0, num_lights=0)):   # the ends of the range are valid
            assert b.call(b.params(2, **ok)) == shim.PT_OK, ok
        assert b.call(b.params(0), lb=None) == shim.PT_OK                     # no lights, no list
        device.waitForCompletion()
    finally:
        b.release()


def test_cut_short_search_is_reported_and_recovers(device, lbvh_scene):
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = lbvh_scene
    assert_cut_short_search_is_reported(
        device, lambda: IndirectRenderer(device, tris, mats, W, H, light_samples=1, max_bounces=3, stripe_rows=1))


def test_empty_scene_renders_the_background(device, cornell):
    from oclpathtracer_amd import scene

    _, mats = cornell
    none = np.zeros(0, scene.TRIANGLE_DTYPE)
    got = _indirect(device, none, mats, W, H, 2, 2, 5, lights=NONE)
    assert_fb_equal(got, io.render(none, mats, W, H, 0, 2, 2, 5, lights=NONE), "empty scene")
    assert np.all(got[:, :3] == got[0, 0]) and got[0, 0] > 0


def test_cpp_harness_indirect_illumination(tmp_path, cornell):
    from oclpathtracer_amd import scene

    tris, mats = cornell
    out, name, pixels = harness_ppm(tmp_path, 32, 3, "IndirectIllumination")
    assert "IndirectIllumination:" in out and name.startswith("indirectIllumination_")
    want = io.render(tris, mats, 32, 32, 0, 3, 1, 16)
    assert np.array_equal(pixels, scene.f2c(want[:, :3]))
