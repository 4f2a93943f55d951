"""Indirect illumination (pt_render_indirect) on the MI355X, bit for bit.

The framebuffer -- and where the workspace holds every frame, the radiance before the fold -- is compared with
tests/indirect_oracle.c, which composes the estimator from the CPU oracle's own steps.  Two identities need no restatement: with no
lights the image is the fused renderer's at the same depth (the second statement of the bounce against pt_shade), at one bounce
it is DirectRenderer's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import indirect_oracle as io
from conftest import ROOT, assert_fb_equal
from gpu_support import SEARCHES, options, render
from indirect_scenes import lbvh_boxes, tiled_boxes
from oclpathtracer_amd import shim
from scenes import GLOSSY_SHIFTS, glossy_room

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int32)
W, H = 40, 24
CASES = ((16, 1), (3, 4))   # (B, K)
FRAMES = 4


def _indirect(device, tris, mats, W, H, frames, K, B, frame_begin=0, want_samples=False, **kw):
    from oclpathtracer_amd.indirect import IndirectRenderer

    kw.setdefault("stripe_rows", 1)
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, **kw)
    try:
        r.render(frames, frame_begin)
        fb = r.read()
        if not want_samples:
            return fb
        assert r.chunk_frames >= frames
        s = np.zeros(3 * r.local_pixels * frames, np.float32)
        r.samples.read(s, len(s))
        device.waitForCompletion()
        return fb, s.reshape(-1, 3)
    finally:
        r.release()


def _want(tris, mats, W, H, frames, K, B, **kw):
    """the restatement's framebuffer and its radiance before the fold, frame-major as the workspace holds it"""
    gid, frame = io.all_samples(W, H, frames)
    return io.render(tris, mats, W, H, 0, frames, K, B, **kw), io.samples(tris, mats, W, H, gid, frame, K, B, **kw)[0]


@pytest.fixture(scope="module")
def cornell_want(cornell):
    """the restatement's images and radiances of the Cornell box: computed once, shared, never written to"""
    tris, mats = cornell
    want = {(B, K): _want(tris, mats, W, H, FRAMES, K, B) for B, K in CASES}
    for fb, rad in want.values():
        fb.setflags(write=False)
        rad.setflags(write=False)
    return want


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
    want_fb, want_rad = _want(tris, mats, W, H, 2, 2, 4)
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
    want_fb, want_rad = _want(tris, mats, W, H, 2, 2, 4)
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
    want_fb, want_rad = _want(tris, mats, W, H, 3, 1, 4)
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
        assert b.call(_params(W, H, len(tris), len(mats), 2), cam=ctypes.byref(bad)) == shim.PT_ERR_INVALID
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
def _params(W, H, ntri, nmat, nl, **kw):
    p = shim.IndirectParams()
    p.width, p.height, p.frame_begin, p.frame_count = W, H, 0, 1
    p.num_triangles, p.num_materials, p.num_lights, p.light_samples = ntri, nmat, nl, 2
    p.stripe_rows, p.n_ranks, p.rank = 1, 1, 0
    p.max_bounces = 3
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


class _Buffers:
    """the buffers of one raw pt_render_indirect call; the framebuffer starts as a sentinel"""

    def __init__(self, device, tris, mats, W, H, lights=(10, 11), pad=4):
        from oclpathtracer_amd import adl, scene

        self.device, self.lib = device, shim.load()
        self.tb = adl.Buffer(device, len(tris), scene.TRIANGLE_DTYPE)
        self.mb = adl.Buffer(device, len(mats), scene.MATERIAL_DTYPE)
        self.lb = adl.Buffer(device, max(len(lights), 1), np.int32)
        self.sb = adl.Buffer(device, 3 * W * H, np.float32)
        self.fb = adl.Buffer(device, W * H + pad, adl.float4)
        self.tb.write(tris, len(tris))
        self.mb.write(mats, len(mats))
        self.lb.write(np.asarray(lights, np.int32), len(lights))
        self.sentinel = np.full((W * H + pad, 4), np.float32(-7.25), np.float32)
        self.fb.write(self.sentinel, len(self.sentinel))

    def call(self, p, cam=None, **over):
        h = lambda name: over[name] if name in over else getattr(self, name)
        ptr = lambda b: b._h if b is not None else None
        return self.lib.pt_render_indirect(self.device._h, ptr(h("tb")), ptr(h("mb")), ptr(h("lb")), ptr(h("sb")), ptr(h("fb")),
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


def test_c_abi_argument_errors_leave_the_framebuffer_untouched(device, cornell):
    from oclpathtracer_amd import adl

    tris, mats = cornell
    Ws, Hs = 16, 8
    ntri, nmat = len(tris), len(mats)
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    b = _Buffers(device, tris, mats, Ws, Hs)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    ob = adl.Buffer(other, 3 * Ws * Hs, np.float32)
    try:
        cases = [(dict(max_bounces=0), E_INV), (dict(max_bounces=65536), E_INV), (dict(max_bounces=-1), E_INV),
                 (dict(reserved=0), E_INV), (dict(reserved=3), E_INV),
                 # direct illumination's list
                 (dict(width=0), E_INV), (dict(height=-1), E_INV), (dict(frame_begin=-1), E_INV), (dict(frame_count=-1), E_INV),
                 (dict(num_triangles=-1), E_INV), (dict(num_materials=0), E_INV), (dict(num_lights=-1), E_INV),
                 (dict(num_lights=1 << 24), E_INV), (dict(light_samples=0), E_INV), (dict(light_samples=257), E_INV),
                 (dict(stripe_rows=0), E_INV), (dict(n_ranks=0), E_INV), (dict(rank=1), E_INV), (dict(rank=-1), E_INV),
                 (dict(frame_begin=0x7fffffff, frame_count=1), E_INV), (dict(width=65536, height=32768), E_INV),
                 (dict(num_triangles=ntri + 1), E_RANGE), (dict(num_materials=nmat + 1), E_RANGE), (dict(num_lights=3), E_RANGE),
                 (dict(width=Ws + 16), E_RANGE)]
        for kw, code in cases:
            assert b.call(_params(Ws, Hs, ntri, nmat, 2, **kw)) == code, kw
        p = _params(Ws, Hs, ntri, nmat, 2)
        assert b.call(None) == E_INV
        for name in ("tb", "mb", "sb", "fb"):
            assert b.call(p, **{name: None}) == E_INV, name
        assert b.call(p, lb=None) == E_INV                                    # num_lights > 0 needs the list
        assert b.call(p, sb=ob) == E_INV                                      # a buffer of another device
        small = adl.Buffer(device, 3 * Ws * Hs - 1, np.float32)
        try:
            assert b.call(p, sb=small) == E_RANGE                             # less than one frame of workspace
        finally:
            small.release()
        bad = shim.Camera()
        b.lib.pt_camera_reference(ctypes.byref(bad))
        bad.fov_y_deg = 180.0
        assert b.call(p, cam=ctypes.byref(bad)) == E_INV
        # a misaligned framebuffer, workspace and framebuffer overlapping: sub-ranges of one allocation
        big = adl.Buffer(device, 64 * Ws * Hs, np.uint8)
        try:
            def wrap(off, nbytes):
                w = adl.Buffer()
                w.setRawPtr(device, big.m_ptr + off, nbytes)
                return w
            f8, s0, f0 = wrap(12 * Ws * Hs + 8, 16 * Ws * Hs), wrap(0, 12 * Ws * Hs), wrap(12 * Ws * Hs - 16, 16 * Ws * Hs)
            try:
                assert b.call(p, sb=s0, fb=f8) == E_INV                       # framebuffer not 16-byte aligned
                assert b.call(p, sb=s0, fb=f0) == E_INV                       # overlap
            finally:
                for w in (f8, s0, f0):
                    w.release()
        finally:
            big.release()
        b.assert_untouched()
        for ok in (dict(max_bounces=1), dict(max_bounces=65535, num_triangles=0, num_lights=0)):   # the ends of the range are valid
            assert b.call(_params(Ws, Hs, ntri, nmat, 2, **ok)) == shim.PT_OK, ok
        assert b.call(_params(Ws, Hs, ntri, nmat, 0), lb=None) == shim.PT_OK   # no lights, no list
        device.waitForCompletion()
    finally:
        b.release()
        ob.release()
        adl.DeviceUtils.deallocate(other)


def test_cut_short_search_is_reported_and_recovers(device, lbvh_scene):
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = lbvh_scene
    with options(device, ACCEL=2):
        d = IndirectRenderer(device, tris, mats, W, H, light_samples=1, max_bounces=3, stripe_rows=1)
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
    exe = os.path.join(ROOT, "oclpathtracer_amd", "raytrace_test")
    scene_path = os.path.join(ROOT, "oclpathtracer_amd", "data", "cornellbox.bin")
    r = subprocess.run([exe, "--only", "IndirectIllumination", "--dim", "32", "--frames", "3", "--scene", scene_path,
                        "--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 1 and "FAILED" not in r.stdout and "IndirectIllumination:" in r.stdout
    ppm = [f for f in os.listdir(tmp_path) if f.endswith(".ppm")]
    assert len(ppm) == 1 and ppm[0].startswith("indirectIllumination_")
    want = io.render(tris, mats, 32, 32, 0, 3, 1, 16)
    toks = open(os.path.join(tmp_path, ppm[0])).read().split()
    assert toks[:4] == ["P3", "32", "32", "255"]
    assert np.array_equal(np.array(toks[4:], np.int64).reshape(-1, 3), scene.f2c(want[:, :3]))
