"""Direct illumination (pt_render_direct) on the MI355X, bit for bit.

The framebuffer is compared with tests/direct_oracle.c, which composes the estimator from the CPU oracle's own camera ray,
triangle test (ascending loop), BRDF expressions and gamma fold; with no lights it is compared with the fused renderer at one
bounce, which needs no restatement."""
import ctypes
from functools import partial

import numpy as np
import pytest

import direct_oracle as do
from conftest import assert_fb_equal
from gpu_support import (SEARCHES, LitBuffers, assert_cut_short_search_is_reported, assert_lit_argument_errors, harness_ppm,
                         lit_with_samples, options, render)
from oclpathtracer_amd import shim
from scenes import edge_scene, nested_boxes

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int32)


def _direct(device, tris, mats, W, H, frames, K, lights=None, camera=None, **kw):
    return lit_with_samples(device, (tris, mats, lights, camera), W, H, frames, K, **kw)[0]


_Buffers = partial(LitBuffers, "pt_render_direct")


def _image(W, H, K):
    tris, mats, _, _ = edge_scene("cornell")[1]
    return (do.render(tris, mats, W, H, 0, 4, K),)


@pytest.fixture(scope="module")
def cornell_want():
    """the restatement's images of the Cornell box, 4 frames: computed once, shared, never written to"""
    return {(W, H, K): do.once(_image, W, H, K)[0] for W, H in ((64, 64), (40, 24)) for K in (1, 4)}


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_bit_exact_against_the_restatement(device, cornell, cornell_want, quad, accel):
    tris, mats = cornell
    for (W, H, K), want in cornell_want.items():
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            got = _direct(device, tris, mats, W, H, 4, K, chunk_frames=3)   # 3 + 1 frames: two launches, two folds
        assert_fb_equal(got, want, "%dx%d K%d q%d a%d" % (W, H, K, quad, accel))


def test_the_comparison_is_not_vacuous(cornell):
    """On the inputs of the test above every kind of light sample occurs: not contributing, occluded, open."""
    tris, mats = cornell
    W = H = 64
    gid = np.arange(W * H)
    hit, dec, _ = do.decisions(tris, mats, W, H, gid, np.zeros(W * H), 4)
    assert hit.all()
    counts = {k: int((dec == k).sum()) for k in (do.NONE, do.OCCLUDED, do.OPEN)}
    print("64x64 frame 0 K 4:", counts)
    assert counts[do.NONE] > 1000 and counts[do.OCCLUDED] > 500 and counts[do.OPEN] > 5000, counts


def test_no_lights_is_the_renderer_at_one_bounce(device, cornell):
    tris, mats = cornell
    W, H = 48, 40
    want = render(device, tris, mats, W, H, 3, depth=1, stripe_rows=1)
    got = _direct(device, tris, mats, W, H, 3, 4, lights=NONE, chunk_frames=2)
    assert_fb_equal(got, want, "no lights against Renderer.render(max_bounces=1)")


def test_progressive_frame_zero_cameras_and_a_rejected_camera(device, cornell):
    from oclpathtracer_amd import adl, scene
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.direct import DirectRenderer

    tris, mats = cornell
    W, H = 48, 32
    want = do.render(tris, mats, W, H, 0, 5, 2)
    r = DirectRenderer(device, tris, mats, W, H, light_samples=2, stripe_rows=1, chunk_frames=2)
    try:
        r.fb.write(np.full((W * H, 4), np.nan, np.float32), W * H)
        r.render(2)                       # frame 0: whatever the buffer held is overwritten
        r.render(3)                       # continues at frame 2: 2 + 1 frames
        assert r.frames_done == 5
        assert_fb_equal(r.read(), want, "progressive")
        r.render(5, 0)
        assert_fb_equal(r.read(), want, "one call, frame_begin 0 overwrites")
    finally:
        r.release()
    cams = [Camera.fit(tris, view_dir=(0.3, -0.4, -1.0), aspect=W / H),
            Camera(eye=(-2.0, 1.0, 3.0), center=(1.0, 3.0, -2.0), up=(0.1, 1.0, 0.0), fov_y_deg=75.0)]
    for i, cam in enumerate(cams):
        assert_fb_equal(_direct(device, tris, mats, W, H, 2, 3, camera=cam), do.render(tris, mats, W, H, 0, 2, 3, cam=cam), "camera %d" % i)
    # a rejected camera enqueues nothing
    lib = shim.load()
    b = _Buffers(device, tris, mats, W, H)
    try:
        bad = shim.Camera()
        lib.pt_camera_reference(ctypes.byref(bad))
        bad.center[:] = bad.eye[:]
        assert b.call(b.params(2), cam=ctypes.byref(bad)) == shim.PT_ERR_INVALID
        b.assert_untouched()
    finally:
        b.release()


def test_stripes_equal_the_single_rank_rows(device, cornell):
    tris, mats = cornell
    W, H, S = 40, 31, 5
    full = _direct(device, tris, mats, W, H, 2, 2, stripe_rows=S).reshape(H, W, 4)
    for R in (2, 3):
        for k in range(R):
            rows = (np.arange(H) // S) % R == k
            got = _direct(device, tris, mats, W, H, 2, 2, stripe_rows=S, n_ranks=R, rank=k)
            assert_fb_equal(got, full[rows], "rank %d of %d" % (k, R))


def test_tiled_brute_force(device):
    tris, mats = nested_boxes(10)          # 360 triangles: the tiled table (257 .. 511), emissive and glossy materials
    assert 257 <= len(tris) <= 511
    W = H = 32
    want = do.render(tris, mats, W, H, 0, 2, 3)
    with options(device, ACCEL=1):
        got = _direct(device, tris, mats, W, H, 2, 3)
    assert_fb_equal(got, want, "tiled brute force")
    _, dec, _ = do.decisions(tris, mats, W, H, np.arange(W * H), np.zeros(W * H), 3)
    assert all((dec == k).any() for k in (do.NONE, do.OCCLUDED, do.OPEN))


@pytest.fixture(scope="module")
def lbvh_scene():
    tris, mats = nested_boxes(15)          # 540 triangles: PT_OPT_ACCEL 0 takes the LBVH
    assert len(tris) >= 512
    return tris, mats


def test_lbvh_against_the_restatement_and_brute_force(device, lbvh_scene):
    tris, mats = lbvh_scene
    W = H = 32
    want = do.render(tris, mats, W, H, 0, 2, 3)
    res = {}
    for accel in (0, 2, 1):
        with options(device, ACCEL=accel):
            res[accel] = _direct(device, tris, mats, W, H, 2, 3)
    assert_fb_equal(res[0], want, "LBVH (automatic) against the restatement")
    assert_fb_equal(res[2], want, "LBVH (forced) against the restatement")
    assert_fb_equal(res[1], res[2], "forced brute force against the LBVH")
    _, dec, _ = do.decisions(tris, mats, W, H, np.arange(W * H), np.zeros(W * H), 3)
    assert all((dec == k).any() for k in (do.NONE, do.OCCLUDED, do.OPEN))


def test_lbvh_refill_over_more_samples_than_the_grid(device, lbvh_scene):
    """768 x 512 = 393 216 samples: more than the persistent grid holds lanes (the direct kernel runs four workgroups of 256 per
    CU, 262 144 lanes on 256 CUs; five, the other driver kernels' figure, would be 327 680), so lanes take further samples."""
    tris, mats = lbvh_scene
    assert 768 * 512 > 256 * 5 * 256
    res = {}
    for accel in (2, 1):
        with options(device, ACCEL=accel):
            res[accel] = _direct(device, tris, mats, 768, 512, 1, 1, chunk_frames=1)
    assert_fb_equal(res[2], res[1], "refill: LBVH against brute force")


# ---- the raw C ABI ------------------------------------------------------------------------------------------------------------
def test_light_indices_out_of_range_are_clamped(device, cornell):
    """Python refuses such a list; through the C ABI it is defined behaviour: each index is clamped into [0, num_triangles)."""
    tris, mats = cornell
    W, H = 32, 24
    ntri = len(tris)
    raw, clamped = [-1, 10, ntri + 5, 11], [0, 10, ntri - 1, 11]
    out = []
    for lights in (raw, clamped):
        b = _Buffers(device, tris, mats, W, H, lights=lights, pad=0)
        try:
            assert b.call(b.params(4)) == shim.PT_OK
            out.append(b.read())
        finally:
            b.release()
    assert_fb_equal(out[0], out[1], "clamped light indices")
    assert_fb_equal(out[1], do.render(tris, mats, W, H, 0, 1, 2, lights=np.array(clamped, np.int32)), "the clamped list")


def test_direct_interleaved_with_renders_and_ao(device, cornell, oracle):
    import ao_oracle
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    W = H = 32
    lib = shim.load()
    with options(device, ACCEL=2, CHUNK_FRAMES=3):
        r = Renderer(device, tris, mats, W, H, want_stats=True, stripe_rows=1)
        a = r.ao_renderer(rays_per_sample=4, radius=0.9)
        dr = r.direct_renderer(light_samples=2, chunk_frames=2)
        try:
            assert dr.lights.tolist() == [10, 11]
            r.render(7)
            dr.render(3)
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            ws = device.getWorkspaceMemory()
            a.render(2)
            r.render(4)
            dr.render(2)
            a.render(2)
            assert_fb_equal(r.read(), oracle.render(tris, mats, W, H, 11), "render around direct and AO renders")
            assert_fb_equal(dr.read(), do.render(tris, mats, W, H, 0, 5, 2), "direct around renders")
            assert np.array_equal(a.read_counts(), ao_oracle.counts(tris, W, H, 0, 4, 4, 0.9))
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds
            assert device.getWorkspaceMemory() == ws
        finally:
            dr.release()
            a.release()
            r.release()


def test_cut_short_search_is_reported_and_recovers(device, lbvh_scene):
    from oclpathtracer_amd.direct import DirectRenderer

    tris, mats = lbvh_scene
    assert_cut_short_search_is_reported(device, lambda: DirectRenderer(device, tris, mats, 48, 48, light_samples=2, stripe_rows=1))


def test_c_abi_argument_errors_leave_the_framebuffer_untouched(device, cornell):
    tris, mats = cornell
    b = _Buffers(device, tris, mats, 16, 8)
    try:
        for k in range(5):
            assert b.call(b.params(2, reserved=k)) == shim.PT_ERR_INVALID, k
        assert_lit_argument_errors(b)
        assert b.call(b.params(2)) == shim.PT_OK
        assert b.call(b.params(0), lb=None) == shim.PT_OK                     # no lights, no list
        device.waitForCompletion()
    finally:
        b.release()


def test_empty_scene_renders_the_background(device, cornell):
    from oclpathtracer_amd import scene

    _, mats = cornell
    got = _direct(device, np.zeros(0, scene.TRIANGLE_DTYPE), mats, 24, 16, 2, 2, lights=NONE)
    want = do.render(np.zeros(0, scene.TRIANGLE_DTYPE), mats, 24, 16, 0, 2, 2, lights=NONE)
    assert_fb_equal(got, want, "empty scene")
    assert np.all(got[:, :3] == got[0, 0]) and got[0, 0] > 0


def test_cpp_harness_direct_illumination(tmp_path, cornell):
    from oclpathtracer_amd import scene

    tris, mats = cornell
    out, name, pixels = harness_ppm(tmp_path, 64, 4, "DirectIllumination")
    assert "DirectIllumination:" in out and name.startswith("directIllumination_")
    want = do.render(tris, mats, 64, 64, 0, 4, 4)
    assert np.array_equal(pixels, scene.f2c(want[:, :3]))
