"""tests/test_gpu_extents.py's sibling: the pixel-list entry points, the features, the lens AO render and the lens rays at the ends of
what the C ABI accepts, against the CPU restatements, bit for bit (assert_fb_equal / np.array_equal: equal bits, equal NaN positions;
no tolerance anywhere).  The inputs and what the restatements say of them are tests/extent_cases.py's; tests/test_extents_cpu.py
proves that each reaches its corner -- every case here names that corner first in its docstring, and its proof carries the name.

The list forms render listed pixels only, so the WIDE row -- 16 777 472 pixels, columns at and above 2^23 -- is affordable for a lit
kernel: its 268 MB framebuffer lives on a device handle of its own, is neither filled nor read whole, and about 900 pixels of it are
listed."""
import ctypes
import time

import numpy as np
import pytest

import adaptive_oracle as ao
import direct_oracle as do
import extent_cases as xc
import feature_oracle as fo
import moments_oracle as mom
from conftest import assert_fb_equal
from env_scenes import env_scene
from gpu_support import options
from oclpathtracer_amd import adl, scene, shim
from oclpathtracer_amd.ao import AORenderer
from oclpathtracer_amd.camera import Camera
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
PAD = 4   # sentinel pixels behind the framebuffer


class Rig:
    """The buffers of raw calls of pt_render_indirect_rr, pt_render_indirect_pixels, pt_render_indirect_pixels_ris, pt_sample_moments and
    pt_sample_moments_pixels on one stripe of an image that may have 2^31 - 64 pixels: the scene, the counts and the light table are an
    IndirectRenderer's (MIS, by power, the roulette of xc.LIST_EST; its own image is 8 x 8 and never rendered); framebuffer (PAD sentinel
    pixels behind it), workspace, list and records are sized for the local pixels and the list."""

    def __init__(self, device, sc, W, H, ws_floats, max_listed, moments=True, **stripes):
        self.device, self.lib = device, shim.load()
        tris, mats, lights, cam = sc
        assert cam is None
        e = xc.LIT[xc.LIST_EST]
        self.sc = IndirectRenderer(device, tris, mats, 8, 8, light_samples=xc.LIT_K, max_bounces=e.B, mis=e.mis, light_choice="power",
                                   roulette=Roulette(*e.rr), lights=lights, chunk_frames=1, stripe_rows=1)
        self.W, self.H, self.stripes = W, H, dict(stripes)
        self.npix = do.local_row_count(H, **stripes) * W
        self.fb = adl.Buffer(device, self.npix + PAD, adl.float4)
        self.sb = adl.Buffer(device, ws_floats, np.float32)
        self.pl = adl.Buffer(device, self.lib.pt_adaptive_list_bytes(max_listed), np.uint8)
        self.mom = adl.Buffer(device, self.npix * mom.MOMENTS_DTYPE.itemsize, np.uint8) if moments else None
        self.ws_floats, self.listed = ws_floats, 0
        self.ris = shim.Ris(xc.LIT_M)

    def params(self, frames, frame_begin=0):
        p = shim.IndirectParams()
        p.width, p.height, p.frame_begin, p.frame_count = self.W, self.H, frame_begin, frames
        p.num_triangles, p.num_materials, p.num_lights = self.sc.num_triangles, self.sc.num_materials, len(self.sc.lights)
        p.light_samples, p.max_bounces = xc.LIT_K, self.sc.max_bounces
        p.stripe_rows, p.n_ranks, p.rank = (self.stripes.get(k, d) for k, d in (("stripe_rows", 1), ("n_ranks", 1), ("rank", 0)))
        return p

    def _head(self):
        s = self.sc
        return (self.device._h, s.tbuf._h, s.mbuf._h, s._lights_h(), *s._estimator(), self.sb._h, self.fb._h)

    def uniform(self, frames, frame_begin=0):
        """pt_render_indirect_rr"""
        return self.lib.pt_render_indirect_rr(*self._head(), ctypes.byref(self.params(frames, frame_begin)), ctypes.byref(self.sc._rr), None, None)

    def set_list(self, pixels, frames):
        s = np.zeros(len(pixels), ao.SLOT_DTYPE)
        s["pixel"], s["frame"] = pixels, frames
        raw = np.frombuffer(np.array([len(s), 0, 0, 0], np.uint32).tobytes() + s.tobytes(), np.uint8)
        self.pl.write(raw, raw.size)
        self.listed = len(s)

    def render_list(self, form, frames, frame_begin=0):
        """pt_render_indirect_pixels or its RIS form over the list of ``set_list``"""
        tail = (self.pl._h, self.listed, ctypes.byref(self.params(frames, frame_begin)), ctypes.byref(self.sc._rr))
        if form == "pixels_ris":
            return self.lib.pt_render_indirect_pixels_ris(*self._head(), *tail, ctypes.byref(self.ris), None, None)
        assert form == "pixels"
        return self.lib.pt_render_indirect_pixels(*self._head(), *tail, None, None)

    def moments_all(self, frames, reset):
        return self.lib.pt_sample_moments(self.device._h, self.sb._h, self.mom._h, self.npix, frames, int(reset), None)

    def moments_list(self, frames):
        return self.lib.pt_sample_moments_pixels(self.device._h, self.sb._h, self.mom._h, self.pl._h, self.listed, frames, None)

    def fill(self, fb=None, records=None):
        """the framebuffer (sentinels behind it, and everywhere without ``fb``), a workspace of sentinels, the records"""
        px = np.full((self.npix + PAD, 4), SENTINEL, np.float32)
        if fb is not None:
            px[:self.npix] = fb
        self.fb.write(px, len(px))
        self.sb.write(np.full(self.ws_floats, SENTINEL, np.float32), self.ws_floats)
        if records is not None:
            self.mom.write(np.ascontiguousarray(records).view(np.uint8), self.mom.getSize())

    def read_fb(self):
        out = np.zeros((self.npix + PAD, 4), np.float32)
        self.fb.read(out, len(out))
        self.device.waitForCompletion()
        return out

    def read_ws(self):
        out = np.zeros(self.ws_floats, np.float32)
        self.sb.read(out, out.size)
        self.device.waitForCompletion()
        return out

    def read_moments(self):
        out = np.zeros(self.mom.getSize(), np.uint8)
        self.mom.read(out, out.size)
        self.device.waitForCompletion()
        return out

    def release(self):
        for b in (self.fb, self.sb, self.pl, self.mom):
            if b is not None:
                b.release()
        self.sc.release()


def _assert_workspace(ws, want, what):
    n = want.size
    assert_fb_equal(ws[:n], want, what + ": radiance before the fold")
    assert np.all(ws[n:] == SENTINEL), what + ": the workspace behind the launch's records was written"


# ---- pixel lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", xc.TALL_LIST_LAYOUTS)
@pytest.mark.parametrize("form", list(xc.LIST_FORMS))
def test_tall_lists_reach_the_last_pixel(device, form, name):
    """TALL lists: a uniform pt_render_indirect_rr of 2 frames and its moments, then 2 frames of every third local pixel and the image's
    last (gid W * H - 1) from frame 2 through the list form, and their moments: the slot's local pixel mapped to its global id through
    the stripe layout at rows up to 2^25 - 2.  THE IDENTITY: the listed pixels hold the uniform restatement's frames 2, 3 folded into
    its frames 0, 1, the others frames 0, 1; unlisted pixels and records are what they were before the call"""
    want_fb0, want_rad0, want_m0, want_ws, want_fb1, want_m1 = xc.list_tall(form, name)
    px = xc.tall_list_pixels(name)
    npix = xc.TALL_ROWS[name] * xc.TALL_W
    for accel in (1, 2):
        what = "%s %s accel %d" % (form, name, accel)
        with options(device, ACCEL=accel):
            b = Rig(device, xc.scene_of("ris_indirect", True), xc.TALL_W, xc.TALL_H, 3 * npix * xc.TALL_LIST_FRAME, len(px), **xc.TALL[name])
            try:
                assert b.npix == npix
                b.fill(records=np.full(b.mom.getSize(), 0xA5, np.uint8))
                assert b.uniform(xc.TALL_LIST_FRAME) == shim.PT_OK, what
                assert b.moments_all(xc.TALL_LIST_FRAME, reset=True) == shim.PT_OK, what
                fb0, m0 = b.read_fb(), b.read_moments()
                _assert_workspace(b.read_ws(), want_rad0, what + ", the uniform start")
                assert_fb_equal(fb0[:npix], want_fb0, what + ", the uniform start")
                assert np.array_equal(m0, want_m0), what + ": the moments of the uniform start"
                b.sb.write(np.full(b.ws_floats, SENTINEL, np.float32), b.ws_floats)
                b.set_list(px, np.full(len(px), xc.TALL_LIST_FRAME))
                assert b.render_list(form, xc.TALL_LIST_FRAMES) == shim.PT_OK, what
                assert b.moments_list(xc.TALL_LIST_FRAMES) == shim.PT_OK, what
                fb1, m1 = b.read_fb(), b.read_moments()
                _assert_workspace(b.read_ws(), want_ws, what)
            finally:
                b.release()
        assert_fb_equal(fb1[px], want_fb1[px], what + ": the listed pixels")
        rest = np.ones(npix + PAD, bool)
        rest[px] = False
        assert fb1[rest].tobytes() == fb0[rest].tobytes(), what + ": a pixel that is not listed was written"
        assert np.all(fb1[npix:] == SENTINEL), what
        assert np.array_equal(m1, want_m1), what + ": %d records differ" % int((m1.reshape(-1, 56) != want_m1.reshape(-1, 56)).any(axis=1).sum())
        assert m1.reshape(-1, 56)[rest[:npix]].tobytes() == m0.reshape(-1, 56)[rest[:npix]].tobytes(), what + ": a record that is not listed was written"


@pytest.mark.parametrize("case,offset", [(c, o) for c, offs in xc.LATE_LIST_OFFSETS.items() for o in offs])
@pytest.mark.parametrize("form", list(xc.LIST_FORMS))
def test_late_lists_wrap_by_the_headers_rule(device, form, case, offset):
    """Wrap (and LATE): all 384 pixels listed, resumed from late_start() and records in hand.  float_ties: slot frame 2^24 - 2, 5
    frames; wrap: slot frame 2^31 - 2, 4 frames -- the numbers are 2^31 - 2, 2^31 - 1, 0, 1 and frame 0 overwrites the pixel, so the
    pixels are the uniform restatement's of frames 0, 1 alone; mixed: slots at 2046 and at 2^31 - 2 alternate, so the lanes of one wave
    sit on both sides of the list fold's reciprocal table's end and of the wrap.  offset: params->frame_begin, the slots' frames that
    much lower -- the same sums, the same pixels"""
    first, frames = xc.LATE_LISTS[case]
    want_ws, want_fb, want_m = xc.list_late(form, case)
    n = xc.LATE_W * xc.LATE_H
    what = "%s %s frame_begin %d" % (form, case, offset)
    b = Rig(device, xc.cornell(), xc.LATE_W, xc.LATE_H, 3 * n * frames + 6, n)
    try:
        b.fill(xc.late_start(), xc.late_moments())
        b.set_list(np.arange(n), first - offset)
        assert b.render_list(form, frames, frame_begin=offset) == shim.PT_OK, what
        assert b.moments_list(frames) == shim.PT_OK, what
        fb, m = b.read_fb(), b.read_moments()
        _assert_workspace(b.read_ws(), want_ws, what)
    finally:
        b.release()
    assert_fb_equal(fb[:n], want_fb, what)
    assert np.all(fb[n:] == SENTINEL), what
    assert np.array_equal(m, want_m), what + ": the moments"


@pytest.fixture(scope="module")
def wide_list_device():
    """a handle of its own for the WIDE list render: its 268 MB framebuffer goes with it; a small staging reservation (the lit
    renders do not stage)"""
    dev = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    dev.reserveStaging(1 << 20)
    yield dev
    adl.DeviceUtils.deallocate(dev)


def _runs(cols):
    """the ascending columns as (first, count) runs of adjacent ones"""
    cuts = np.flatnonzero(np.diff(cols) != 1) + 1
    return [(int(r[0]), len(r)) for r in np.split(cols, cuts)]


def _read_pixels(b, cols):
    out = np.zeros((len(cols), 4), np.float32)
    k = 0
    for first, n in _runs(cols):
        b.fb.read(out[k: k + n], n, first)
        k += n
    b.device.waitForCompletion()
    return out


def test_wide_list_reaches_the_window(wide_list_device):
    """WIDE list: one local row of 16 777 472 pixels; the window about the centre (columns at and above 2^23, where a jittered x is a
    neighbouring column's), both ends of the row and 512 scattered columns listed at frame 0, 4 frames, MIS, by power: the listed
    pixels are roulette_oracle.samples and the fold at those gids; the two pixels on either side of each block keep their sentinels"""
    dev = wide_list_device
    cols, guards = xc.wide_list_columns(), xc.wide_sentinel_columns()
    want_ws, want_px = xc.wide_list()
    t0 = time.perf_counter()
    b = Rig(dev, xc.cornell(), xc.WIDE_W, xc.WIDE_H, 3 * len(cols) * xc.WIDE_LIST_FRAMES + 6, len(cols), moments=False, **xc.WIDE_STRIPES)
    try:
        assert b.npix == xc.WIDE_W
        mark = np.full((1, 4), SENTINEL, np.float32)
        for c in guards:
            b.fb.write(mark, 1, int(c))
        b.sb.write(np.full(b.ws_floats, SENTINEL, np.float32), b.ws_floats)
        b.set_list(cols, np.zeros(len(cols)))
        with options(dev, ACCEL=1):
            assert b.render_list("pixels", xc.WIDE_LIST_FRAMES) == shim.PT_OK
        got, kept = _read_pixels(b, cols), _read_pixels(b, np.sort(guards))
        ws = b.read_ws()
    finally:
        b.release()
    print("the WIDE list case took %.2f s on the device and its host, allocation and release included" % (time.perf_counter() - t0))
    _assert_workspace(ws, want_ws, "WIDE list")
    for name, first, n in xc.wide_columns()[0] + [("every listed", 0, xc.WIDE_W)]:
        at = (cols >= first) & (cols < first + n)
        print("%s columns: %d of %d pixels differ from the restatement's" % (
            name, int((got[at].view(np.uint32) != want_px[at].view(np.uint32)).any(axis=1).sum()), int(at.sum())))
    assert_fb_equal(got, want_px, "WIDE list: the listed pixels")
    assert np.all(kept == SENTINEL), "a pixel beside a listed block was written"


# ---- the features ------------------------------------------------------------------------------------------------------------------
class FeatureRig:
    """four outputs of ``frames`` frames of npix local pixels, each with a guard word behind it and filled with the guard's value"""

    def __init__(self, device, tris, mats, W, H, frames, **stripes):
        self.device, self.lib = device, shim.load()
        self.W, self.H, self.frames, self.stripes = W, H, frames, stripes
        self.ntri, self.nmat = len(tris), len(mats)
        self.npix = fo.local_pixels(W, H, **stripes)
        self.tb = adl.Buffer(device, len(tris), scene.TRIANGLE_DTYPE)
        self.mb = adl.Buffer(device, len(mats), scene.MATERIAL_DTYPE)
        self.tb.write(np.ascontiguousarray(tris), len(tris))
        self.mb.write(np.ascontiguousarray(mats), len(mats))
        self.words = 3 * self.npix * frames
        self.out = {f: adl.Buffer(device, self.words + 1, np.float32) for f in fo.FEATURES}
        for o in self.out.values():
            o.write(np.full(self.words + 1, SENTINEL, np.float32), self.words + 1)

    def call(self, frames, frame_begin, cam):
        p = shim.FeatureParams()
        p.width, p.height, p.frame_begin, p.frame_count = self.W, self.H, frame_begin, frames
        p.num_triangles, p.num_materials = self.ntri, self.nmat
        p.stripe_rows, p.n_ranks, p.rank = (self.stripes.get(k, d) for k, d in (("stripe_rows", 1), ("n_ranks", 1), ("rank", 0)))
        s = Camera.struct_of(cam)
        return self.lib.pt_render_features(self.device._h, self.tb._h, self.mb._h, *[self.out[f]._h for f in fo.FEATURES], ctypes.byref(p),
                                           ctypes.byref(s) if s is not None else None, None)

    def read(self):
        out = {}
        for f in fo.FEATURES:
            out[f] = np.zeros(self.words + 1, np.float32)
            self.out[f].read(out[f], self.words + 1)
        self.device.waitForCompletion()
        return out

    def release(self):
        for b in [self.tb, self.mb] + list(self.out.values()):
            b.release()


def _assert_features(got, want, npix, frames, what):
    for f in fo.FEATURES:
        assert_fb_equal(got[f][:-1].reshape(frames, npix, 3), getattr(want, f), "%s: %s" % (what, f))
        assert got[f][-1] == SENTINEL, "%s: the guard word behind %s was written" % (what, f)


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("name", list(xc.TALL))
def test_features_tall(device, name, lens):
    """TALL: pt_render_features, item f * npix + lp of four outputs, at global rows up to 2^25 - 2 -- hits and misses, under the plain
    camera and under the lens camera; the guard word behind each output stays"""
    tris, mats = xc.feature_scene(True)
    want = xc.features_tall(name, lens)
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            b = FeatureRig(device, tris, mats, xc.TALL_W, xc.TALL_H, xc.FEATURE_FRAMES, **xc.TALL[name])
            try:
                assert b.call(xc.FEATURE_FRAMES, 0, xc.lens_camera() if lens else None) == shim.PT_OK
                got = b.read()
            finally:
                b.release()
        _assert_features(got, want, xc.TALL_ROWS[name] * xc.TALL_W, xc.FEATURE_FRAMES, "%s lens %d accel %d" % (name, lens, accel))


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_features_late(device, lens):
    """LATE: pt_render_features at frames 2^31 - 4 .. 2^31 - 2, all outputs; one frame more is refused with PT_ERR_INVALID (frame_begin +
    frame_count above 2^31 - 1) and nothing is written"""
    tris, mats = xc.feature_scene(False)
    frame_begin, frames = xc.LATE["last_frames"]
    want = xc.features_late(lens)
    cam = xc.lens_camera() if lens else None
    n = xc.LATE_W * xc.LATE_H
    b = FeatureRig(device, tris, mats, xc.LATE_W, xc.LATE_H, frames + 1)
    try:
        assert b.call(frames + 1, frame_begin, cam) == shim.PT_ERR_INVALID
        for f, a in b.read().items():
            assert np.all(a == SENTINEL), "%s was written by a call that was refused" % f
        assert b.call(frames, frame_begin, cam) == shim.PT_OK
        got = b.read()
    finally:
        b.release()
    for f in fo.FEATURES:
        assert_fb_equal(got[f][:3 * n * frames].reshape(frames, n, 3), getattr(want, f), "lens %d: %s" % (lens, f))
        assert np.all(got[f][3 * n * frames:] == SENTINEL), "lens %d: %s was written behind its samples" % (lens, f)


# ---- the lens: ambient occlusion and pt_camera_rays ------------------------------------------------------------------------------------
def _ao(device, tris, W, H, frames, frame_begin=0, **stripes):
    r = AORenderer(device, tris, W, H, rays_per_sample=xc.AO_K, radius=xc.AO_RADIUS, camera=xc.lens_camera(), **stripes)
    try:
        r.counts.write(np.zeros(2 * max(r.local_pixels, 1), np.uint32), 2 * r.local_pixels)
        r.render(frames, frame_begin)
        return r.read_counts()
    finally:
        r.release()


@pytest.mark.parametrize("name", list(xc.TALL))
def test_ao_lens_tall(device, name):
    """Lens, TALL: pt_render_ao's counts under the lens camera at gids up to W * H - 1"""
    tris = env_scene(xc.TALL_SCENE)[0]
    want = xc.ao_lens_tall(name)
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            got = _ao(device, tris, xc.TALL_W, xc.TALL_H, 2, **xc.TALL[name])
        assert np.array_equal(got, want), "%s accel %d: %d counts differ" % (name, accel, int((got != want).sum()))


def test_lens_late(device):
    """Lens, LATE: pt_render_ao's counts at frames 2^31 - 4 .. 2^31 - 2 and pt_camera_rays at frame 2^31 - 2, under the lens camera"""
    from oclpathtracer_amd.query import RayCaster

    tris = xc.cornell()[0]
    frame_begin, frames = xc.LATE["last_frames"]
    want = xc.ao_lens_late()
    got = _ao(device, tris, xc.LATE_W, xc.LATE_H, frames, frame_begin, stripe_rows=1)
    assert np.array_equal(got, want), "%d counts differ" % int((got != want).sum())
    rc = RayCaster(device, tris)
    try:
        rays = rc.camera_rays(xc.LATE_W, xc.LATE_H, xc.LENS_RAYS_FRAME, xc.lens_camera())
    finally:
        rc.release()
    got = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)
    assert_fb_equal(got[:, :7], xc.lens_rays_late()[:, :7], "origins, tmax and directions at frame 2^31 - 2")
