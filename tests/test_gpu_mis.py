"""Indirect illumination with multiple importance sampling (pt_render_indirect_mis, pt_light_counts) on the MI355X, bit for bit.

Every case of tests/mis_cases.py -- at most 40 x 24 x 3 frames per call -- is compared twice with tests/mis_oracle.c, NaN masks
equal: the sample workspace with the radiance before the fold, and the framebuffer.  tests/test_mis_cpu.py proves, on these very
inputs, that weighted, last-vertex and back-side light samples and later hits on emitters with counts of 0, 1 and 2 all occur, and
that no sample holds a NaN.  The identities need no restatement: with no lights the image is the fused renderer's, at one bounce it
is DirectRenderer's, and a plain IndirectRenderer beside a MIS one is unmoved."""
from functools import partial

import numpy as np
import pytest

import indirect_oracle as io
import mis_cases as mc
import mis_oracle as mo
from conftest import assert_fb_equal
from gpu_support import SEARCHES, LitBuffers, assert_lit_argument_errors, harness_ppm, lit_with_samples, options, render
from indirect_edges import clamped_raw
from oclpathtracer_amd import shim
from scenes import edge_scene

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int32)
W, H, FRAMES = mc.W, mc.H, mc.FRAMES


_Buffers = partial(LitBuffers, "pt_render_indirect_mis")


def _mis(device, scene, lights, Ws, Hs, frames, K, B, **kw):
    """one IndirectRenderer(mis=True) on a named scene, one render: (framebuffer, workspace [chunk_frames, local pixels, 3])"""
    tris, mats, _, cam = edge_scene(scene)[1]
    return lit_with_samples(device, (tris, mats, mc.lights_of(scene, lights), cam), Ws, Hs, frames, K, max_bounces=B, mis=True, **kw)


def _compare(device, scene, lights, Ws, Hs, frames, K, B, what, **stripes):
    want_fb, want_rad = mc.wanted(scene, lights, Ws, Hs, frames, K, B, **stripes)
    fb, ws = _mis(device, scene, lights, Ws, Hs, frames, K, B, **stripes)
    assert_fb_equal(ws[:frames], want_rad, what + ": radiance before the fold")
    assert_fb_equal(fb, want_fb, what)


# ---- every search --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_every_search_on_the_cornell_box(device, quad, accel):
    """brute force with the table in LDS and the LBVH forced on the 36-triangle scene, under every filter"""
    for K, B in mc.SEARCH_KB:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            _compare(device, "cornell", None, W, H, FRAMES, K, B, "K%d B%d q%d a%d" % (K, B, quad, accel))


def test_tiled_brute_force(device):
    name, K, B = mc.BIG[0]
    assert 257 <= len(edge_scene(name)[1][0]) <= 511
    with options(device, ACCEL=1):
        _compare(device, name, None, W, H, FRAMES, K, B, "tiled brute force")


@pytest.mark.parametrize("accel", [0, 2, 1])
def test_lbvh_and_forced_brute_force(device, accel):
    name, K, B = mc.BIG[1]
    assert len(edge_scene(name)[1][0]) >= 512
    with options(device, ACCEL=accel):
        _compare(device, name, None, W, H, FRAMES, K, B, "540 triangles, accel %d" % accel)


# ---- parameters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,B", mc.PARAM_KB)
def test_light_samples_and_bounces(device, K, B):
    _compare(device, "cornell", None, W, H, FRAMES, K, B, "K%d B%d" % (K, B))


@pytest.mark.parametrize("name,K,B", mc.FINITE)
def test_finite_glossy_rooms(device, name, K, B):
    """every vertex a GGX one: pbl's quotient at every finite roughness"""
    _compare(device, name, None, W, H, FRAMES, K, B, name)
    with options(device, ACCEL=2):
        _compare(device, name, None, W, H, FRAMES, K, B, name + " through the LBVH")


@pytest.mark.parametrize("name", mc.SMALL_SCENES)
def test_small_images(device, name):
    """1, 15 and 65 pixels: one sample; one partial wave; a full wave and one lane -- lanes ending at different vertices"""
    for Ws, Hs, B in mc.SMALL:
        for accel in (1, 2):
            with options(device, ACCEL=accel):
                _compare(device, name, None, Ws, Hs, 2, 4, B, "%s %dx%d accel %d" % (name, Ws, Hs, accel))


def test_three_rank_stripes(device):
    _compare(device, "cornell", None, W, H, 2, 1, 4, "one rank, stripes of %d rows" % mc.STRIPE_ROWS, stripe_rows=mc.STRIPE_ROWS)
    for r in range(mc.RANKS):
        _compare(device, "cornell", None, W, H, 2, 1, 4, "rank %d of %d" % (r, mc.RANKS), stripe_rows=mc.STRIPE_ROWS, n_ranks=mc.RANKS, rank=r)


def test_chunks_and_a_resumed_call(device, cornell):
    from oclpathtracer_amd.indirect import IndirectRenderer

    K, B = 1, 4
    want3 = mc.wanted("cornell", None, W, H, FRAMES, K, B)[0]
    one = _mis(device, "cornell", None, W, H, FRAMES, K, B, chunk_frames=1)[0]
    assert_fb_equal(one, want3, "a workspace of one frame: three launches, three folds")
    tris, mats = cornell
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, mis=True, stripe_rows=1, chunk_frames=FRAMES)
    try:
        r.fb.write(np.full((W * H, 4), np.nan, np.float32), W * H)
        r.render(FRAMES)                  # frame 0: whatever the buffer held is overwritten
        assert_fb_equal(r.read(), want3, "the first call")
        r.render(FRAMES)                  # resumes at frame_begin = 3
        assert r.frames_done == 2 * FRAMES
        assert_fb_equal(r.read(), mc.wanted("cornell", None, W, H, 2 * FRAMES, K, B)[0], "a second call resuming at frame 3")
    finally:
        r.release()


# ---- lists -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.LISTS))
def test_light_lists(device, name):
    """the emitters, a duplicated entry, an emitter missing, a wall in the list, unsorted: the counts 0, 1 and 2 at later hits"""
    K, B = mc.LIST_KB
    _compare(device, "cornell", name, W, H, FRAMES, K, B, "list %s" % name)
    with options(device, ACCEL=2):
        _compare(device, "cornell", name, W, H, FRAMES, K, B, "list %s through the LBVH" % name)


# ---- the raw C ABI ---------------------------------------------------------------------------------------------------------------
def test_indices_out_of_range_are_clamped_in_list_and_counts(device, cornell):
    """[-1, 10, ntri + 5, 11] through the C ABI, the counts made by pt_light_counts from that same list: the image of [0, 10, 35, 11]"""
    tris, mats = cornell
    K, B = mc.LIST_KB
    raw = clamped_raw(len(tris))
    want_fb, want_rad = mc.wanted("cornell", "clamped", W, H, FRAMES, K, B)
    b = _Buffers(device, tris, mats, W, H, lights=raw, frames=FRAMES, pad=0)
    try:
        assert b.read(b.cb, np.zeros(len(tris), np.int32)).tolist() == mo.light_counts(raw, len(tris)).tolist()
        p = b.params(len(raw), frame_count=FRAMES, light_samples=K, max_bounces=B)
        assert b.call(p) == shim.PT_OK
        assert_fb_equal(b.read(), want_fb, "clamped list")
        assert_fb_equal(b.read(b.sb, np.zeros((FRAMES * W * H, 3), np.float32)), want_rad.reshape(-1, 3), "clamped list: radiance before the fold")
    finally:
        b.release()


def test_light_counts_against_bincount(device, cornell):
    from oclpathtracer_amd import adl

    tris, _ = cornell
    ntri = len(tris)
    lib = shim.load()
    rng = np.random.default_rng(5)
    lists = [NONE, np.array([10, 11], np.int32), np.asarray(clamped_raw(ntri), np.int32), rng.integers(0, ntri, ntri).astype(np.int32),
             rng.integers(-5, ntri + 5, 1000).astype(np.int32)]   # (the last: four blocks, many lanes on one counter)
    cb = adl.Buffer(device, ntri, np.int32)
    try:
        for li in lists:
            lb = adl.Buffer(device, max(len(li), 1), np.int32)
            try:
                if len(li):
                    lb.write(li, len(li))
                cb.write(np.full(ntri, -3, np.int32), ntri)     # what the buffer held is cleared
                for _ in range(2):                              # twice: the same result
                    assert lib.pt_light_counts(device._h, lb._h if len(li) else None, len(li), ntri, cb._h, None) == shim.PT_OK
                    got = np.zeros(ntri, np.int32)
                    cb.read(got, ntri)
                    device.waitForCompletion()
                    assert got.tolist() == np.bincount(np.clip(li, 0, ntri - 1), minlength=ntri).tolist(), li
            finally:
                lb.release()
        # errors, the counts untouched
        cb.write(np.full(ntri, -3, np.int32), ntri)
        lb = adl.Buffer(device, 2, np.int32)
        small = adl.Buffer(device, ntri - 1, np.int32)
        try:
            E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
            assert lib.pt_light_counts(device._h, lb._h, 2, ntri, None, None) == E_INV
            assert lib.pt_light_counts(device._h, None, 2, ntri, cb._h, None) == E_INV
            assert lib.pt_light_counts(device._h, lb._h, -1, ntri, cb._h, None) == E_INV
            assert lib.pt_light_counts(device._h, lb._h, 2, -1, cb._h, None) == E_INV
            assert lib.pt_light_counts(device._h, lb._h, 1 << 24, ntri, cb._h, None) == E_INV
            assert lib.pt_light_counts(device._h, lb._h, 3, ntri, cb._h, None) == E_RANGE
            assert lib.pt_light_counts(device._h, lb._h, 2, ntri, small._h, None) == E_RANGE
            assert lib.pt_light_counts(device._h, cb._h, 2, ntri, cb._h, None) == E_INV      # overlap
            got = np.zeros(ntri, np.int32)
            cb.read(got, ntri)
            device.waitForCompletion()
            assert (got == -3).all()
        finally:
            lb.release()
            small.release()
    finally:
        cb.release()


# ---- device identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 16])
def test_no_lights_and_null_counts_is_the_renderer(device, cornell, B):
    tris, mats = cornell
    want = render(device, tris, mats, W, H, FRAMES, depth=B, stripe_rows=1)
    b = _Buffers(device, tris, mats, W, H, frames=FRAMES, pad=0)
    try:
        p = b.params(0, frame_count=FRAMES, light_samples=4, max_bounces=B)
        assert b.call(p, lb=None, cb=None) == shim.PT_OK
        assert_fb_equal(b.read(), want, "no lights, NULL counts against Renderer.render(max_bounces=%d)" % B)
    finally:
        b.release()
    from oclpathtracer_amd.indirect import IndirectRenderer

    r = IndirectRenderer(device, tris, mats, W, H, light_samples=4, max_bounces=B, mis=True, lights=NONE, stripe_rows=1, chunk_frames=2)
    try:
        r.render(FRAMES)
        assert_fb_equal(r.read(), want, "IndirectRenderer(mis=True, lights=[]) against Renderer.render(max_bounces=%d)" % B)
    finally:
        r.release()


@pytest.mark.parametrize("K", [1, 4])
def test_one_bounce_is_direct_illumination(device, cornell, K):
    from oclpathtracer_amd.direct import DirectRenderer

    tris, mats = cornell
    d = DirectRenderer(device, tris, mats, W, H, light_samples=K, stripe_rows=1)
    try:
        d.render(FRAMES)
        want = d.read()
    finally:
        d.release()
    assert_fb_equal(_mis(device, "cornell", None, W, H, FRAMES, K, 1)[0], want, "B = 1 against DirectRenderer, K = %d" % K)


def test_a_plain_renderer_beside_a_mis_one_is_unmoved(device, cornell):
    """both over one Renderer's buffers, renders interleaved: the plain one is still indirect_oracle's, the MIS one mis_oracle's"""
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    K, B = 1, 4
    r = Renderer(device, tris, mats, W, H, stripe_rows=1)
    plain = r.indirect_renderer(light_samples=K, max_bounces=B, chunk_frames=FRAMES)
    mis = r.indirect_renderer(light_samples=K, max_bounces=B, chunk_frames=FRAMES, mis=True)
    try:
        assert mis.mis and not plain.mis and plain.counts is None and mis.counts is not None and mis.lights.tolist() == [10, 11]
        mis.render(2)
        plain.render(FRAMES)
        mis.render(1)
        assert_fb_equal(plain.read(), io.render(tris, mats, W, H, 0, FRAMES, K, B), "mis=False beside mis=True")
        assert_fb_equal(mis.read(), mc.wanted("cornell", None, W, H, FRAMES, K, B)[0], "mis=True beside mis=False")
    finally:
        mis.release()
        plain.release()
        r.release()
    assert mis.counts is None


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_framebuffer_untouched(device, cornell):
    from oclpathtracer_amd import adl

    tris, mats = cornell
    Ws, Hs = 16, 8
    ntri = len(tris)
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    b = _Buffers(device, tris, mats, Ws, Hs)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    oc = adl.Buffer(other, ntri, np.int32)
    short = adl.Buffer(device, ntri - 1, np.int32)
    big = adl.Buffer(device, 12 * Ws * Hs + 4 * ntri + 16, np.uint8)
    try:
        p = b.params(2)
        assert b.call(p, cb=None) == E_INV                                    # NULL counts with nl > 0
        assert b.call(p, cb=short) == E_RANGE                                 # one triangle short
        assert b.call(p, cb=oc) == E_INV                                      # counts of another device

        def wrap(off, nbytes):
            w = adl.Buffer()
            w.setRawPtr(device, big.m_ptr + off, nbytes)
            return w
        s0, c_in, c_odd = wrap(0, 12 * Ws * Hs), wrap(12 * Ws * Hs - 8, 4 * ntri), wrap(12 * Ws * Hs + 2, 4 * ntri)
        try:
            assert b.call(p, sb=s0, cb=c_in) == E_INV                         # counts overlapping the workspace
            assert b.call(p, sb=s0, cb=c_odd) == E_INV                        # counts not 4-byte aligned
        finally:
            for w in (s0, c_in, c_odd):
                w.release()
        assert b.call(p, cb=b.lb) == E_RANGE                                  # (the list as counts: too small before it overlaps)
        for kw in [dict(max_bounces=0), dict(max_bounces=65536), dict(max_bounces=-1)] + [dict(reserved=k) for k in range(4)]:
            assert b.call(b.params(2, **kw)) == E_INV, kw
        assert_lit_argument_errors(b)                                         # what every entry point rejects, the framebuffer untouched
        for ok in (dict(max_bounces=1), dict(max_bounces=65535, num_triangles=0, num_lights=0)):   # the ends of the range are valid
            assert b.call(b.params(2, **ok)) == shim.PT_OK, ok
        device.waitForCompletion()
    finally:
        b.release()
        oc.release()
        short.release()
        big.release()
        adl.DeviceUtils.deallocate(other)


def test_cpp_harness_mis(tmp_path, cornell):
    from oclpathtracer_amd import scene

    tris, mats = cornell
    out, name, pixels = harness_ppm(tmp_path, 32, 3, "IndirectIllumination", "--mis")
    assert "IndirectIllumination (MIS):" in out and name.startswith("indirectIllumination_") and name.endswith("_mis.ppm")
    want = mo.render(tris, mats, 32, 32, 0, 3, 1, 16)
    assert np.array_equal(pixels, scene.f2c(want[:, :3]))
