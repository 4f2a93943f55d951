"""Direct illumination (pt_render_direct) on the MI355X, bit for bit.

The framebuffer is compared with tests/direct_oracle.c, which composes the estimator from the CPU oracle's own camera ray,
triangle test (ascending loop), BRDF expressions and gamma fold; with no lights it is compared with the fused renderer at one
bounce, which needs no restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import direct_oracle as do
from conftest import ROOT, assert_fb_equal
from gpu_support import SEARCHES, options, render
from oclpathtracer_amd import shim
from scenes import nested_boxes

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int32)


def _direct(device, tris, mats, W, H, frames, K, frame_begin=0, **kw):
    from oclpathtracer_amd.direct import DirectRenderer

    kw.setdefault("stripe_rows", 1)
    r = DirectRenderer(device, tris, mats, W, H, light_samples=K, **kw)
    try:
        r.render(frames, frame_begin)
        return r.read()
    finally:
        r.release()


@pytest.fixture(scope="module")
def cornell_want(cornell):
    """the restatement's images of the Cornell box, 4 frames: computed once, shared, never written to"""
    tris, mats = cornell
    want = {(W, H, K): do.render(tris, mats, W, H, 0, 4, K) for W, H in ((64, 64), (40, 24)) for K in (1, 4)}
    for a in want.values():
        a.setflags(write=False)
    return want


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
        assert b.call(_params(W, H, len(tris), len(mats), 2), cam=ctypes.byref(bad)) == shim.PT_ERR_INVALID
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
def _params(W, H, ntri, nmat, nl, **kw):
    p = shim.DirectParams()
    p.width, p.height, p.frame_begin, p.frame_count = W, H, 0, 1
    p.num_triangles, p.num_materials, p.num_lights, p.light_samples = ntri, nmat, nl, 2
    p.stripe_rows, p.n_ranks, p.rank = 1, 1, 0
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


class _Buffers:
    """the buffers of one raw pt_render_direct call; the framebuffer starts as a sentinel"""

    def __init__(self, device, tris, mats, W, H, lights=(10, 11), frames=1, pad=4):
        from oclpathtracer_amd import adl, scene

        self.device, self.lib, self.n = device, shim.load(), W * H
        self.tb = adl.Buffer(device, len(tris), scene.TRIANGLE_DTYPE)
        self.mb = adl.Buffer(device, len(mats), scene.MATERIAL_DTYPE)
        self.lb = adl.Buffer(device, max(len(lights), 1), np.int32)
        self.sb = adl.Buffer(device, 3 * W * H * frames, np.float32)
        self.fb = adl.Buffer(device, W * H + pad, adl.float4)
        self.tb.write(tris, len(tris))
        self.mb.write(mats, len(mats))
        if len(lights):
            self.lb.write(np.asarray(lights, np.int32), len(lights))
        self.sentinel = np.full((W * H + pad, 4), np.float32(-7.25), np.float32)
        self.fb.write(self.sentinel, len(self.sentinel))

    def call(self, p, cam=None, **over):
        h = lambda name: over[name] if name in over else getattr(self, name)
        ptr = lambda b: b._h if b is not None else None
        return self.lib.pt_render_direct(self.device._h, ptr(h("tb")), ptr(h("mb")), ptr(h("lb")), ptr(h("sb")), ptr(h("fb")),
                                         ctypes.byref(p) if p is not None else None, cam, None)

    def read(self):
        out = np.zeros_like(self.sentinel)
        self.fb.read(out, len(out))
        self.device.waitForCompletion()
        return out

    def assert_untouched(self):
        assert np.array_equal(self.read(), self.sentinel), "the framebuffer was touched"

    def release(self):
        for b in (self.tb, self.mb, self.lb, self.sb, self.fb):
            b.release()


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
            assert b.call(_params(W, H, ntri, len(mats), 4)) == shim.PT_OK
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
    with options(device, ACCEL=2):
        d = DirectRenderer(device, tris, mats, 48, 48, light_samples=2, stripe_rows=1)
        try:
            d.render(1)
            want = d.read()
            with options(device, BVH_STACK_LIMIT=1):
                with pytest.raises(shim.ShimError) as e:   # the search is cut short; the observing call reports it
                    d.render(1, 0)
                    d.read()
                assert e.value.code == shim.PT_ERR_TRAVERSAL
            device.waitForCompletion()                     # the word was cleared by the report
            d.render(1, 0)
            assert_fb_equal(d.read(), want, "after the report")
        finally:
            d.release()


def test_c_abi_argument_errors_leave_the_framebuffer_untouched(device, cornell):
    from oclpathtracer_amd import adl

    tris, mats = cornell
    W, H = 16, 8
    ntri, nmat = len(tris), len(mats)
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    b = _Buffers(device, tris, mats, W, H)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    ob = adl.Buffer(other, 3 * W * H, np.float32)
    try:
        cases = [(dict(width=0), E_INV), (dict(height=-1), E_INV), (dict(frame_begin=-1), E_INV), (dict(frame_count=-1), E_INV),
                 (dict(num_triangles=-1), E_INV), (dict(num_materials=0), E_INV), (dict(num_lights=-1), E_INV),
                 (dict(num_lights=1 << 24), E_INV), (dict(light_samples=0), E_INV), (dict(light_samples=257), E_INV),
                 (dict(stripe_rows=0), E_INV), (dict(n_ranks=0), E_INV), (dict(rank=1), E_INV), (dict(rank=-1), E_INV),
                 (dict(reserved=0), E_INV), (dict(reserved=4), E_INV), (dict(frame_begin=0x7fffffff, frame_count=1), E_INV),
                 (dict(width=65536, height=32768), E_INV),
                 (dict(num_triangles=ntri + 1), E_RANGE), (dict(num_materials=nmat + 1), E_RANGE), (dict(num_lights=3), E_RANGE),
                 (dict(width=W + 16), E_RANGE)]
        for kw, code in cases:
            assert b.call(_params(W, H, ntri, nmat, 2, **kw)) == code, kw
        p = _params(W, H, ntri, nmat, 2)
        assert b.call(None) == E_INV
        for name in ("tb", "mb", "sb", "fb"):
            assert b.call(p, **{name: None}) == E_INV, name
        assert b.call(p, lb=None) == E_INV                                    # num_lights > 0 needs the list
        assert b.call(p, sb=ob) == E_INV                                      # a buffer of another device
        small = adl.Buffer(device, 3 * W * H - 1, np.float32)
        try:
            assert b.call(p, sb=small) == E_RANGE                             # less than one frame of workspace
        finally:
            small.release()
        bad = shim.Camera()
        b.lib.pt_camera_reference(ctypes.byref(bad))
        bad.fov_y_deg = 180.0
        assert b.call(p, cam=ctypes.byref(bad)) == E_INV
        # a misaligned framebuffer, workspace and framebuffer overlapping: sub-ranges of one allocation
        big = adl.Buffer(device, 64 * W * H, np.uint8)
        try:
            def wrap(off, nbytes):
                w = adl.Buffer()
                w.setRawPtr(device, big.m_ptr + off, nbytes)
                return w
            f8, s0, f0 = wrap(12 * W * H + 8, 16 * W * H), wrap(0, 12 * W * H), wrap(12 * W * H - 16, 16 * W * H)
            try:
                assert b.call(p, sb=s0, fb=f8) == E_INV                       # framebuffer not 16-byte aligned
                assert b.call(p, sb=s0, fb=f0) == E_INV                       # overlap
            finally:
                for w in (f8, s0, f0):
                    w.release()
        finally:
            big.release()
        b.assert_untouched()
        assert b.call(p) == shim.PT_OK
        assert b.call(_params(W, H, ntri, nmat, 0), lb=None) == shim.PT_OK     # no lights, no list
        device.waitForCompletion()
    finally:
        b.release()
        ob.release()
        adl.DeviceUtils.deallocate(other)


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
    exe = os.path.join(ROOT, "oclpathtracer_amd", "raytrace_test")
    scene_path = os.path.join(ROOT, "oclpathtracer_amd", "data", "cornellbox.bin")
    r = subprocess.run([exe, "--only", "DirectIllumination", "--dim", "64", "--frames", "4", "--scene", scene_path,
                        "--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 1 and "FAILED" not in r.stdout and "DirectIllumination:" in r.stdout
    ppm = [f for f in os.listdir(tmp_path) if f.endswith(".ppm")]
    assert len(ppm) == 1 and ppm[0].startswith("directIllumination_")
    want = do.render(tris, mats, 64, 64, 0, 4, 4)
    toks = open(os.path.join(tmp_path, ppm[0])).read().split()
    assert toks[:4] == ["P3", "64", "64", "255"]
    assert np.array_equal(np.array(toks[4:], np.int64).reshape(-1, 3), scene.f2c(want[:, :3]))
