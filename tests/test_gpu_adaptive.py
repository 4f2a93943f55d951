"""Adaptive sampling (pt_adaptive_select, pt_render_indirect_pixels, pt_sample_moments_pixels, IndirectRenderer.render_adaptive) on the
MI355X, bit for bit: NaN positions equal, equal bits elsewhere.

The list kernels are compared with their parents (a full list at one common frame is pt_render_indirect_rr), with the restatement
(tests/roulette_oracle.c: a slot's samples are roulette_oracle.samples of its pixel and its own frames, its framebuffer pixel
roulette_oracle.render after as many frames as the pixel has received), and the whole loop with tests/adaptive_oracle.py's.  The inputs
are tests/adaptive_cases.py's, images of a few hundred pixels; tests/test_adaptive_cpu.py proves on these very inputs that the loop
reaches its edges."""
import ctypes

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_oracle as ao
import direct_oracle as do
import moments_oracle as mom
import roulette_cases as rc
import roulette_oracle as ro
from adaptive_support import PixelBuffers, _expect, _list_bytes, _run_list, _scattered, _slots
from conftest import assert_fb_equal
from gpu_support import SEARCHES, assert_lit_argument_errors, options
from oclpathtracer_amd import adl, scene, shim
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette
from scenes import edge_scene

pytestmark = pytest.mark.gpu

E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE


# ---- 1. select alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ac.PATTERNS)
def test_select_on_uploaded_records(device, pattern):
    lib = shim.load()
    rule = shim.AdaptiveRule(ac.RULE.tol2, ac.RULE.floor2, ac.RULE.min_samples, ac.RULE.max_samples)
    for pixels in ac.select_sizes():
        m, want_active = ac.select_records(pixels, pattern)
        nbytes = lib.pt_adaptive_list_bytes(pixels)
        assert nbytes >= 16 + 8 * pixels and nbytes % 8 == 0
        mb, lb = adl.Buffer(device, pixels * 56, np.uint8), adl.Buffer(device, nbytes, np.uint8)
        try:
            mb.write(m.view(np.uint8), m.nbytes)
            lb.write(np.full(nbytes, 0xA5, np.uint8), nbytes)
            assert lib.pt_adaptive_select(device._h, mb._h, pixels, ctypes.byref(rule), lb._h, None) == shim.PT_OK
            got, after = np.zeros(16 + 8 * pixels, np.uint8), np.zeros(m.nbytes, np.uint8)
            lb.read(got, got.size)
            mb.read(after, after.size)
            device.waitForCompletion()
            want = ao.select(m, ac.RULE)
            what = "%d pixels, %s" % (pixels, pattern)
            assert got[:16].view(np.uint32).tolist() == [len(want), 0, 0, 0], what
            slots = got[16: 16 + 8 * len(want)].view(ao.SLOT_DTYPE)
            assert np.array_equal(slots["pixel"], want["pixel"]), what + ": pixels"
            assert np.array_equal(slots["frame"], want["frame"]), what + ": frames"
            assert len(want) == int(want_active.sum())
            assert after.tobytes() == m.tobytes(), what + ": the moments were written"
        finally:
            mb.release()
            lb.release()


def test_select_of_no_pixels_writes_an_empty_header(device):
    lib = shim.load()
    assert lib.pt_adaptive_list_bytes(0) == 16
    rule = shim.AdaptiveRule(0.0, 0.0, 1, 1)
    mb, lb = adl.Buffer(device, 56, np.uint8), adl.Buffer(device, 16, np.uint8)
    try:
        lb.write(np.full(16, 0xA5, np.uint8), 16)
        assert lib.pt_adaptive_select(device._h, mb._h, 0, ctypes.byref(rule), lb._h, None) == shim.PT_OK
        got = np.ones(16, np.uint8)
        lb.read(got, 16)
        device.waitForCompletion()
        assert not got.any()
    finally:
        mb.release()
        lb.release()


# ---- 2. the list kernels equal their parents ----------------------------------------------------------------------------------------
PARENT_SCENES = (("cornell", 1, 6), rc.TILED, rc.GLOSSY, rc.LBVH)


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_a_full_list_at_one_frame_is_the_parent(device, quad, accel):
    """every pixel listed at frame z0, F frames: pt_render_indirect_rr over [z0, z0 + F), workspace and framebuffer, for the four
    estimators with a roulette that is played and one that never is"""
    W, H, z0, F = 24, 16, 5, 3
    rng = np.random.default_rng(11)
    with options(device, QUAD_FILTER=quad, ACCEL=accel):
        for name, K, B in PARENT_SCENES:
            b = PixelBuffers(device, edge_scene(name)[1], W, H, frames=F)
            try:
                fb0 = b.sentinel.copy()
                fb0[:W * H] = rng.uniform(0.0, 1.0, (W * H, 4)).astype(np.float32)
                b.full_list(W * H, z0)
                for mis, power in rc.ESTIMATORS:
                    for R, cap in ((1, 0.25), (ro.NEVER, 1.0)):
                        what = "q%d a%d %s mis %d power %d R %d" % (quad, accel, name, mis, power, R)
                        b.estimator(mis, power)
                        b.fb.write(fb0, len(fb0))
                        assert b.rr(b.params(b.nl, frame_begin=z0, frame_count=F, light_samples=K, max_bounces=B), rr=b.roulette(R, cap)) == shim.PT_OK, what
                        want_ws, want_fb = b.workspace(), b.read()
                        b.fb.write(fb0, len(fb0))
                        b.sb.write(b.ws_sentinel, b.ws_sentinel.size)
                        assert b.call(b.params(b.nl, frame_count=F, light_samples=K, max_bounces=B), rr=b.roulette(R, cap)) == shim.PT_OK, what
                        assert_fb_equal(b.workspace(), want_ws, what + ": radiance before the fold")
                        assert_fb_equal(b.read(), want_fb, what)
                        assert not np.array_equal(want_fb[:W * H], fb0[:W * H])
            finally:
                b.release()


# ---- 3. scattered lists with mixed frames -----------------------------------------------------------------------------------------
SCATTER = ("cornell", 24, 16, 1, 8, 1, 0.25, True, False)   # (scene, W, H, K, B, R, cap, mis, power)


def _list_shape(n, npix):
    """(listed, F) with listed * F == n, as many frames (at most 5) as divide n and leave the list inside the image"""
    for F in (5, 4, 3, 2, 1):
        if n % F == 0 and n // F <= npix:
            return n // F, F
    raise AssertionError(n)


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("n", rc.refill_counts(), ids=lambda n: "n%d" % n)
def test_scattered_lists_with_mixed_frames(device, n, accel):
    name, W, H, K, B, R, cap, mis, power = SCATTER
    listed, F = _list_shape(n, W * H)
    assert listed * F == n
    slots = _scattered(np.random.default_rng(n), W * H, listed)
    with options(device, ACCEL=accel):
        b = PixelBuffers(device, edge_scene(name)[1], W, H, frames=5)
        try:
            _run_list(device, b, name, W, H, slots, F, K, B, R, cap, mis, power, "%d x %d items, accel %d" % (listed, F, accel))
        finally:
            b.release()


@pytest.mark.parametrize("mis,power", rc.ESTIMATORS, ids=rc.EST_IDS)
def test_scattered_lists_under_every_estimator(device, mis, power):
    name, W, H, K, B, R, cap = "cornell", 24, 16, 2, 6, 2, 0.5
    for accel in (1, 2):
        slots = _scattered(np.random.default_rng(accel), W * H, 101)
        with options(device, ACCEL=accel):
            b = PixelBuffers(device, edge_scene(name)[1], W, H, frames=3)
            try:
                _run_list(device, b, name, W, H, slots, 3, K, B, R, cap, mis, power, "accel %d" % accel)
                _run_list(device, b, name, W, H, slots, 3, K, B, B, cap, mis, power, "no roulette, accel %d" % accel)
            finally:
                b.release()


def test_scattered_lists_on_the_tiled_table_and_on_the_lbvh(device):
    for (name, K, B), accel in ((rc.TILED, 1), (rc.LBVH, 0)):
        slots = _scattered(np.random.default_rng(5), 24 * 16, 3 * 64 + 7, max_frame=3)
        with options(device, ACCEL=accel):
            b = PixelBuffers(device, edge_scene(name)[1], 24, 16, frames=2)
            try:
                _run_list(device, b, name, 24, 16, slots, 2, K, B, 1, 0.25, True, True, "%s accel %d" % (name, accel))
            finally:
                b.release()


# ---- 4. edge cases of one list render ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
def test_stripes_over_three_ranks(device, accel):
    name, W, H, K, B, R, cap, mis, power = "cornell", 24, 19, 1, 6, 1, 0.5, True, True
    with options(device, ACCEL=accel):
        for rank in range(3):
            st = dict(stripe_rows=3, n_ranks=3, rank=rank)
            npix = do.local_row_count(H, **st) * W
            slots = _scattered(np.random.default_rng(rank), npix, 70, max_frame=3)
            b = PixelBuffers(device, edge_scene(name)[1], W, H, frames=2)
            try:
                _run_list(device, b, name, W, H, slots, 2, K, B, R, cap, mis, power, "rank %d of 3, accel %d" % (rank, accel), **st)
            finally:
                b.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_a_workspace_smaller_than_the_frames_of_the_list(device, accel):
    """50 slots, 5 frames, a workspace of two frames of the list: three launches and three folds; the workspace keeps the last chunk"""
    name, W, H, K, B, R, cap, mis, power = SCATTER
    slots = _scattered(np.random.default_rng(50), W * H, 50)
    want_ws, want_px, start = _expect(name, W, H, slots, 5, K, B, R, cap, mis, power)
    with options(device, ACCEL=accel):
        b = PixelBuffers(device, edge_scene(name)[1], W, H).estimator(mis, power)
        small = adl.Buffer(device, 2 * 50 * 3 + 2, np.float32)   # (two frames of the list and two floats)
        try:
            fb0 = b.sentinel.copy()
            fb0[slots["pixel"]] = start
            b.fb.write(fb0, len(fb0))
            b.set_list(slots)
            assert b.call(b.params(b.nl, frame_count=5, light_samples=K, max_bounces=B), rr=b.roulette(R, cap), sb=small) == shim.PT_OK
            ws = np.zeros((2, 50, 3), np.float32)
            small.read(ws, ws.size)
            assert_fb_equal(b.read()[slots["pixel"]], want_px, "2 + 2 + 1 frames")
            assert_fb_equal(ws[0], want_ws[4], "the workspace holds the last chunk")
            assert_fb_equal(ws[1], want_ws[3], "and what the chunk before left behind it")
        finally:
            small.release()
            b.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_a_frame_begin_offset_and_a_slot_at_frame_zero(device, accel):
    name, W, H, K, B, R, cap, mis, power = SCATTER
    slots = _scattered(np.random.default_rng(9), W * H, 40, max_frame=4)
    with options(device, ACCEL=accel):
        b = PixelBuffers(device, edge_scene(name)[1], W, H, frames=3)
        try:
            _run_list(device, b, name, W, H, slots, 3, K, B, R, cap, mis, power, "offset 2", offset=2)
            zero = _slots(slots["pixel"], np.zeros(len(slots)))
            _run_list(device, b, name, W, H, zero, 3, K, B, R, cap, mis, power, "every slot at frame 0")   # (over a framebuffer of zeros; then:)
            b.fb.write(b.sentinel, len(b.sentinel))
            assert b.call(b.params(b.nl, frame_count=3, light_samples=K, max_bounces=B), rr=b.roulette(R, cap)) == shim.PT_OK
            want = _expect(name, W, H, zero, 3, K, B, R, cap, mis, power)[1]
            assert_fb_equal(b.read()[zero["pixel"]], want, "frame 0 overwrites the pixel: the sentinel is not read")
        finally:
            b.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_frames_that_straddle_the_reciprocal_table(device, accel):
    """8 x 8 pixels at frame 2046, four frames: the fold's tabulated 1 / z ends at 2047; against a uniform device render of 2050"""
    W = H = 8
    K, B, R, cap = 1, 4, 2, 0.5
    with options(device, ACCEL=accel):
        b = PixelBuffers(device, edge_scene("cornell")[1], W, H, frames=64).estimator(True, False)
        try:
            rr = b.roulette(R, cap)
            assert b.rr(b.params(b.nl, frame_count=2050, light_samples=K, max_bounces=B), rr=rr) == shim.PT_OK
            want = b.read()
            assert b.rr(b.params(b.nl, frame_count=2046, light_samples=K, max_bounces=B), rr=rr) == shim.PT_OK
            b.full_list(W * H, 2046)
            assert b.call(b.params(b.nl, frame_count=4, light_samples=K, max_bounces=B), rr=rr) == shim.PT_OK
            assert_fb_equal(b.read(), want, "frames 2046 .. 2049 through the list")
        finally:
            b.release()


def test_an_out_of_range_slot_is_clamped(device):
    name, W, H, K, B, R, cap, mis, power = SCATTER
    npix = W * H
    for bad in (npix, npix + 5, 0xFFFFFFFF):
        slots = _slots([3, bad, 77], [2, 1, 0])
        clamped = _slots([3, npix - 1, 77], [2, 1, 0])
        want_ws, want_px, start = _expect(name, W, H, clamped, 2, K, B, R, cap, mis, power)
        for accel in (1, 2):
            with options(device, ACCEL=accel):
                b = PixelBuffers(device, edge_scene(name)[1], W, H, frames=2).estimator(mis, power)
                try:
                    fb0 = b.sentinel.copy()
                    fb0[clamped["pixel"]] = start
                    b.fb.write(fb0, len(fb0))
                    b.set_list(slots)
                    assert b.call(b.params(b.nl, frame_count=2, light_samples=K, max_bounces=B), rr=b.roulette(R, cap)) == shim.PT_OK
                    fb = b.read()
                    assert_fb_equal(b.workspace()[:18], want_ws, "slot %d: radiance" % bad)
                    assert_fb_equal(fb[clamped["pixel"]], want_px, "slot %d: the last pixel takes it" % bad)
                    fb[clamped["pixel"]] = fb0[clamped["pixel"]]
                    assert fb.tobytes() == fb0.tobytes(), "slot %d: something else was written" % bad
                finally:
                    b.release()


def test_argument_errors_of_the_list_render(device, cornell):
    tris, mats = cornell
    W, H = 16, 8
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    b = PixelBuffers(device, (tris, mats, (10, 11), None), W, H)
    ol = adl.Buffer(other, 16 + 8 * W * H, np.uint8)
    big = adl.Buffer(device, 64 * W * H, np.uint8)
    try:
        b.full_list(W * H, 0)
        p = b.params(2)
        assert b.call(p, pl=None) == E_INV                                   # a NULL list
        assert b.call(p, num_listed=W * H + 1) == E_INV                      # more slots than local pixels
        assert b.call(p, pl=ol) == E_INV                                     # a list of another device
        assert b.call(p, rr=None) == E_INV
        assert b.call(p, rr=b.roulette(first_bounce=0)) == E_INV and b.call(p, rr=b.roulette(reserved=1)) == E_INV
        assert b.call(p, mis=2) == E_INV

        def wrap(off, nbytes, dtype=np.uint8):
            w = adl.Buffer(dtype=dtype)
            w.setRawPtr(device, big.m_ptr + off, nbytes // np.dtype(dtype).itemsize)
            return w
        short, odd = wrap(0, 16 + 8 * W * H - 8), wrap(4, 16 + 8 * W * H)
        s0, l0 = wrap(4096, 12 * W * H, np.float32), wrap(4096 + 12 * W * H - 8, 16 + 8 * W * H)
        try:
            assert b.call(p, pl=short) == E_RANGE                            # a slot short
            assert b.call(p, pl=short, num_listed=W * H - 1) == shim.PT_OK
            assert b.call(p, pl=odd) == E_INV                                # not 8-byte aligned
            assert b.call(p, sb=s0, pl=l0) == E_INV                          # the list overlaps the workspace
        finally:
            for w in (short, odd, s0, l0):
                w.release()
        b.fb.write(b.sentinel, len(b.sentinel))
        assert b.call(b.params(2, frame_count=0)) == shim.PT_OK and b.call(p, num_listed=0) == shim.PT_OK   # nothing is enqueued
        b.assert_untouched()
        assert_lit_argument_errors(b)                                        # what every lit entry point rejects
    finally:
        big.release()
        ol.release()
        b.release()
        adl.DeviceUtils.deallocate(other)


def test_argument_errors_of_select_and_of_the_list_moments(device):
    lib = shim.load()
    n = 100
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    mb, lb = adl.Buffer(device, n * 56, np.uint8), adl.Buffer(device, lib.pt_adaptive_list_bytes(n), np.uint8)
    sb = adl.Buffer(device, 3 * n * 2, np.float32)
    om = adl.Buffer(other, n * 56, np.uint8)
    big = adl.Buffer(device, 32768, np.uint8)
    m = ac.select_records(n, "every_other")[0]
    mb.write(m.view(np.uint8), m.nbytes)

    def wrap(off, nbytes):
        w = adl.Buffer()
        w.setRawPtr(device, big.m_ptr + off, nbytes)
        return w
    wraps = []
    try:
        def rule(tol2=0.25, floor2=0.5, reserved=None):
            r = shim.AdaptiveRule(tol2, floor2, 4, 64)
            if reserved is not None:
                r.reserved[reserved] = 1
            return ctypes.byref(r)

        def select(moments=mb, pixels=n, r="default", lst=lb):
            return lib.pt_adaptive_select(device._h, moments._h if moments else None, pixels, rule() if r == "default" else r, lst._h if lst else None, None)
        assert select(moments=None) == E_INV and select(lst=None) == E_INV and select(r=None) == E_INV
        for bad in (dict(tol2=-1.0), dict(tol2=float("nan")), dict(floor2=-0.5), dict(floor2=float("nan")), dict(reserved=0), dict(reserved=1)):
            assert select(r=rule(**bad)) == E_INV, bad
        assert select(r=rule(tol2=-0.0, floor2=float("inf"))) == shim.PT_OK
        assert select(moments=om) == E_INV                                   # another device's buffer
        assert select(pixels=n + 1) == E_RANGE
        m8, l4, l_short = wrap(4, n * 56), wrap(4, lib.pt_adaptive_list_bytes(n)), wrap(0, lib.pt_adaptive_list_bytes(n) - 1)
        m0, l_over = wrap(8192, n * 56), wrap(8192 + n * 56 - 8, lib.pt_adaptive_list_bytes(n))
        wraps += [m8, l4, l_short, m0, l_over]
        assert select(moments=m8) == E_INV and select(lst=l4) == E_INV      # alignment
        assert select(lst=l_short) == E_RANGE
        assert select(moments=m0, lst=l_over) == E_INV                       # overlap

        assert select() == shim.PT_OK
        listed = len(ao.select(m, ac.RULE))

        def moments(samples=sb, mo=mb, lst=lb, k=listed, frames=2):
            return lib.pt_sample_moments_pixels(device._h, samples._h if samples else None, mo._h if mo else None, lst._h if lst else None, k, frames, None)
        assert moments(samples=None) == E_INV and moments(mo=None) == E_INV and moments(lst=None) == E_INV
        assert moments(frames=-1) == E_INV
        assert moments(k=n + 1) == E_INV                                     # more slots than records
        assert moments(mo=om) == E_INV
        assert moments(k=n, frames=3) == E_RANGE                             # the samples of 3 frames of 100 slots do not fit
        s_odd = adl.Buffer(dtype=np.float32)
        s_odd.setRawPtr(device, big.m_ptr + 16384 + 2, 3 * n * 2 - 1)
        wraps.append(s_odd)
        assert moments(samples=s_odd, k=10) == E_INV                         # alignment
        assert moments(mo=m8) == E_INV and moments(lst=l4) == E_INV
        wraps.append(wrap(0, 16 + 8 * listed - 1))
        assert moments(lst=wraps[-1]) == E_RANGE
        assert moments(mo=m0, lst=l_over) == E_INV                           # overlap
        assert moments(frames=0) == shim.PT_OK and moments(k=0) == shim.PT_OK
        after = np.zeros(m.nbytes, np.uint8)
        mb.read(after, after.size)
        device.waitForCompletion()
        assert after.tobytes() == m.tobytes(), "the moments were touched"
    finally:
        for w in wraps:
            w.release()
        for x in (mb, lb, sb, om, big):
            x.release()
        adl.DeviceUtils.deallocate(other)


# ---- 5. pt_sample_moments_pixels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("listed,frames", [(1, 1), (63, 3), (257, 9), (300, 4)])
def test_the_moments_of_a_scattered_list(device, listed, frames):
    lib = shim.load()
    npix = 24 * 16
    rng = np.random.default_rng(listed)
    s = (rng.uniform(1.0, 3.4, (frames, listed, 3)) * 10.0 ** rng.integers(-20, 20, (frames, listed, 3))).astype(np.float32)
    f, j = np.nonzero(rng.uniform(size=(frames, listed)) < 0.1)
    s[f, j, rng.integers(0, 3, len(f))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(f))
    start = mom.accumulate((rng.uniform(0, 2, (5, npix, 3)) * 10.0 ** rng.integers(-20, 20, (5, npix, 3))).astype(np.float32))
    start["n"][:4] = 0xFFFFFFFF
    slots = _scattered(rng, npix, listed)
    raw = _list_bytes(slots)
    sb, mb, lb = adl.Buffer(device, s.size, np.float32), adl.Buffer(device, npix * 56, np.uint8), adl.Buffer(device, raw.size, np.uint8)
    try:
        sb.write(s, s.size)
        mb.write(start.view(np.uint8), start.nbytes)
        lb.write(raw, raw.size)
        assert lib.pt_sample_moments_pixels(device._h, sb._h, mb._h, lb._h, listed, frames, None) == shim.PT_OK
        got = mom.zeros(npix)
        mb.read(got.view(np.uint8), got.nbytes)
        device.waitForCompletion()
        want = start.copy()
        want[slots["pixel"]] = mom.accumulate(s, start[slots["pixel"]])
        assert got.tobytes() == want.tobytes(), "%d slots, %d frames: %d records differ" % (listed, frames, int((got != want).sum()))
        assert int(got["rejected"].sum()) > int(start["rejected"].sum()) or listed == 1
    finally:
        for x in (sb, mb, lb):
            x.release()


# ---- 6. the whole loop --------------------------------------------------------------------------------------------------------------
class _Recorder:
    """the library with the list length of every pt_render_indirect_pixels call"""

    def __init__(self, lib):
        self._lib, self.listed = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "pt_render_indirect_pixels":
            return fn

        def call(*a):
            self.listed.append(int(a[11]))
            return fn(*a)
        return call


@pytest.mark.parametrize("name", sorted(ac.LOOPS))
def test_render_adaptive_is_the_restated_loop(device, name):
    scene_name, W, H, K, B, R, cap, mis, kw = ac.LOOPS[name]
    tris, mats, lights, cam = edge_scene(scene_name)[1]
    want = ac.loop(name)
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, mis=mis, roulette=Roulette(R, cap), moments=True,
                         stripe_rows=1, chunk_frames=2)
    try:
        r._lib = rec = _Recorder(r._lib)
        got = r.render_adaptive(**kw)
        r._lib = rec._lib
        assert got.passes == want.passes, name
        calls = [n for i, n in enumerate(rec.listed) if i == 0 or n != rec.listed[i - 1]]
        assert calls == list(want.passes), "the list length of every pt_render_indirect_pixels call"
        assert got.samples == int(want.counts.sum())
        assert np.array_equal(got.counts, want.counts) and np.array_equal(r.sample_counts(), want.counts)
        m = mom.zeros(W * H)
        r.mom.read(m.view(np.uint8), m.nbytes)
        device.waitForCompletion()
        assert m.tobytes() == want.moments.tobytes(), "%s: %d moment records differ" % (name, int((m != want.moments).sum()))
        assert_fb_equal(r.read(), want.fb, name)
        assert r.noise().samples == int(want.moments["n"].sum())
        assert r.render_adaptive(**kw).passes == ()                       # nothing is left to do
        for args in ((1,), (1, 5), (1, r.frames_done)):
            with pytest.raises(ValueError):
                r.render(*args)
        r.render(2, 0)                                                   # from frame 0 the pixels share a frame number again
        assert_fb_equal(r.read(), ro.render(tris, mats, W, H, 0, 2, K, B, R, cap, mis=mis), "a fresh start")
        r.render(1)
        assert r.frames_done == 3 and np.array_equal(r.sample_counts(), np.full(W * H, 3, np.uint32))
    finally:
        r.release()


def test_render_adaptive_without_roulette_and_by_power(device, cornell):
    """a renderer without roulette plays none (first_bounce 65535); tolerance 0 lists every pixel until max_samples: the uniform image"""
    tris, mats = cornell
    W, H, K, B = 16, 8, 1, 4
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, mis=True, light_choice="power", moments=True,
                         stripe_rows=1, chunk_frames=3)
    try:
        kw = dict(tolerance=0.0, min_samples=2, max_samples=7, frames_per_pass=3, floor=0.0)
        want = ao.loop((tris, mats, None, None), W, H, K, B, ro.NEVER, 1.0, mis=True, power=True, **kw)
        got = r.render_adaptive(**kw)
        assert got.passes == want.passes and len(got.passes) == 2 and np.array_equal(got.counts, want.counts)
        assert int(got.counts.max()) == 8 and (got.counts == 8).sum() > W * H // 2                        # 2 + 3 + 3: the cap is tested on entry
        assert_fb_equal(r.read(), want.fb, "tolerance 0")
        with pytest.raises(ValueError):
            r.render_adaptive(-1.0, max_samples=8)
    finally:
        r.release()
    d = IndirectRenderer(device, tris, mats, W, H, max_bounces=B)
    try:
        with pytest.raises(RuntimeError):
            d.render_adaptive(0.1, max_samples=8)
    finally:
        d.release()


# ---- the C++ harness -------------------------------------------------------------------------------------------------------------
def test_cpp_harness_adaptive(tmp_path, cornell):
    from gpu_support import harness_ppm

    tris, mats = cornell
    dim, kw = 24, dict(tolerance=0.25, min_samples=8, max_samples=40, frames_per_pass=8)
    want = ao.loop((tris, mats, None, None), dim, dim, 1, 16, 3, 0.95, mis=True, **kw)
    out, name, pixels = harness_ppm(tmp_path, dim, 40, "IndirectIllumination", "--roulette", "3", "--mis", "--adaptive", "0.25,8", "--noise")
    assert name.endswith("_mis_rr_adaptive.ppm"), name
    line = [l for l in out.splitlines() if l.startswith("adaptive:")][0]
    assert line == "adaptive: tolerance 0.25 min 8 max 40 passes [%s] samples %d" % (" ".join(str(n) for n in want.passes), int(want.counts.sum())), line
    assert len(want.passes) >= 2 and 0 < want.passes[-1] < want.passes[0] < dim * dim
    assert np.array_equal(pixels, scene.f2c(want.fb[:, :3]))
    noise = [l for l in out.splitlines() if l.startswith("noise:")][0].split()
    assert int(noise[noise.index("samples") + 1]) + int(noise[noise.index("rejected") + 1]) == int(want.counts.sum())
