"""The thin lens on the device, bit for bit against its restatement (tests/lens_oracle.py; NaN masks equal): every estimator that starts
its samples one by one, on the three searches, from two lens cameras; the shapes at which a sample start goes wrong; pt_camera_rays; the
pinhole identities; a wild lens; what is refused."""
import ctypes
import math

import numpy as np
import pytest

import ao_oracle
import direct_oracle as do
import lens_oracle as lo
import lens_support as ls
import roulette_oracle
from adaptive_support import PixelBuffers, _slots
from conftest import assert_fb_equal
from gpu_support import LitBuffers, harness_ppm, options
from oclpathtracer_amd import adl, scene, shim
from oclpathtracer_amd import ao as ao_mod
from oclpathtracer_amd.camera import Camera

pytestmark = pytest.mark.gpu

W, H, FRAMES = 24, 16, 2
# (search, camera): both cameras on the table in LDS and on the LBVH, the oblique one on the tiled table
SEARCH_CAMERAS = [("lds", "reference"), ("lds", "oblique"), ("tiled", "oblique"), ("lbvh", "reference"), ("lbvh", "oblique")]


def _scene(search):
    make, accel = ls.SEARCH_SCENES[search]
    return make() + (accel,)


def _compare(got, want, what):
    fb, ws = got
    wfb, wws = want[0], want[1]
    assert_fb_equal(ws, wws, what + ": radiance before the fold")
    assert_fb_equal(fb, wfb, what + ": framebuffer")


@pytest.mark.parametrize("est", ls.ESTIMATORS, ids=lambda e: e.name)
@pytest.mark.parametrize("search,camera", SEARCH_CAMERAS)
def test_estimators(device, search, camera, est):
    tris, mats, accel = _scene(search)
    cam = ls.CAMERAS[camera]()
    want = ls.oracle_render(tris, mats, est, cam, W, H, FRAMES)
    with options(device, ACCEL=accel):
        got = ls.gpu_render(device, tris, mats, est, cam, W, H, FRAMES)
    _compare(got, want, "%s, %s, %s" % (est.name, search, camera))


def _ao(device, tris, cam, w, h, frames, frame_begin=0, Kao=4, radius=1.5, **stripes):
    r = ao_mod.AORenderer(device, tris, w, h, rays_per_sample=Kao, radius=radius, camera=cam, stripe_rows=stripes.pop("stripe_rows", 1), **stripes)
    try:
        if frame_begin:
            r.render(frame_begin, 0)
        r.render(frames, frame_begin)
        return r.read_counts(), r.read_image()
    finally:
        r.release()


@pytest.mark.parametrize("search,camera", SEARCH_CAMERAS)
def test_ambient_occlusion(device, search, camera):
    tris, _, accel = _scene(search)
    cam = ls.CAMERAS[camera]()
    want = ls.ao_counts(tris, cam, W, H, 0, FRAMES, 4, 1.5)
    with options(device, ACCEL=accel):
        counts, image = _ao(device, tris, cam, W, H, FRAMES)
    assert np.array_equal(counts, want), "%s, %s: counts differ at %d pixels" % (search, camera, int((counts != want).any(-1).sum()))
    assert want[..., 1].sum() > 0 and want[..., 0].sum() > 0
    a = ao_mod.resolve(want, 4).reshape(-1)
    assert_fb_equal(image[:, 0], a, "AO image")
    pin = ao_oracle.counts(tris, W, H, 0, FRAMES, 4, 1.5, cam=cam)
    assert not np.array_equal(pin, want), "the lens changed nothing: the test would pass for a pinhole"


# ---- pt_render_indirect_pixels: a hand-made list of out-of-order pixels at frame numbers of their own ---------------------------------
@pytest.mark.parametrize("search,camera", [("lds", "oblique"), ("lbvh", "reference")])
def test_pixel_list(device, search, camera):
    tris, mats, accel = _scene(search)
    cam = ls.CAMERAS[camera]()
    w, h, F = 16, 8, 2
    slots = _slots([77, 3, 127, 0, 64, 65, 9, 100, 31], [4, 0, 2, 7, 0, 1, 3, 0, 5])
    R, cap = ls.RR
    gid = np.tile(slots["pixel"].astype(np.int32), F)
    frame = (slots["frame"].astype(np.int32)[None, :] + np.arange(F, dtype=np.int32)[:, None]).reshape(-1)
    with lo.lens(*lo.lens_of(cam)):
        want = roulette_oracle.samples(tris, mats, w, h, gid, frame, ls.K, ls.B, R, cap, mis=True, power=True, cam=cam)[0]
    b = PixelBuffers(device, (tris, mats, None, None), w, h, frames=F)
    try:
        b.estimator(True, True).set_list(slots)
        p = b.params(b.nl, frame_begin=0, frame_count=F, light_samples=ls.K, max_bounces=ls.B)
        cs = Camera.struct_of(cam)
        with options(device, ACCEL=accel):
            assert b.call(p, cam=ctypes.byref(cs), rr=b.roulette(R, cap)) == shim.PT_OK
            ws = b.workspace()
        n = F * len(slots) * 3
        assert_fb_equal(ws[:n], want, "every slot's samples, %s" % search)
        assert np.array_equal(ws[n:], b.ws_sentinel[n:]), "the workspace behind the launch's records was written"
    finally:
        b.release()


# ---- the shapes at which a sample start goes wrong --------------------------------------------------------------------------------------
SHAPE_ESTIMATORS = ["direct_power", "indirect_rr"]


@pytest.mark.parametrize("est", SHAPE_ESTIMATORS)
@pytest.mark.parametrize("search", ["lds", "lbvh"])
@pytest.mark.parametrize("w,h", [(1, 1), (15, 1), (13, 5)])
def test_small_images(device, search, est, w, h):
    """1, 15 and 65 pixels: one lane, a partial wave, a wave plus one lane"""
    tris, mats, accel = _scene(search)
    est, cam = ls.BY_NAME[est], ls.oblique_lens()
    want = ls.oracle_render(tris, mats, est, cam, w, h, 3)
    with options(device, ACCEL=accel):
        got = ls.gpu_render(device, tris, mats, est, cam, w, h, 3)
        counts, _ = _ao(device, tris, cam, w, h, 3)
    _compare(got, want, "%s %dx%d %s" % (est.name, w, h, search))
    assert np.array_equal(counts, ls.ao_counts(tris, cam, w, h, 0, 3, 4, 1.5)), "AO counts %dx%d %s" % (w, h, search)


@pytest.mark.parametrize("est", SHAPE_ESTIMATORS)
@pytest.mark.parametrize("search", ["lds", "lbvh"])
def test_frame_begin_and_chunks(device, search, est):
    """frames [5, 7) on the restatement's image of frames [0, 5), and a render cut into calls of 3 + 1 frames"""
    tris, mats, accel = _scene(search)
    est, cam = ls.BY_NAME[est], ls.reference_lens()
    want = ls.oracle_render(tris, mats, est, cam, W, H, 2, frame_begin=5)
    whole = ls.oracle_render(tris, mats, est, cam, W, H, 1, frame_begin=3)   # the image after 4 frames, the samples of the last
    with options(device, ACCEL=accel):
        got = ls.gpu_render(device, tris, mats, est, cam, W, H, 2, frame_begin=5, fb_init=want[2])
        cut = ls.gpu_render(device, tris, mats, est, cam, W, H, 3, chunks=[3, 1])
        counts, _ = _ao(device, tris, cam, W, H, 2, frame_begin=5)
    _compare(got, want, "%s from frame 5, %s" % (est.name, search))
    _compare(cut, whole, "%s in 3 + 1 frames, %s" % (est.name, search))
    assert np.array_equal(counts, ls.ao_counts(tris, cam, W, H, 0, 7, 4, 1.5)), "AO counts of frames [0, 5) + [5, 7)"


@pytest.mark.parametrize("est", SHAPE_ESTIMATORS)
def test_stripes(device, est):
    """three ranks, stripes of 4 rows, a 40 x 24 image: each rank's share against the one-rank restatement"""
    tris, mats, accel = _scene("lbvh")
    est, cam = ls.BY_NAME[est], ls.oblique_lens()
    w, h = 40, 24
    wfb, wws, _ = ls.oracle_render(tris, mats, est, cam, w, h, 1)
    wao = ls.ao_counts(tris, cam, w, h, 0, 1, 4, 1.5).reshape(-1, 2)
    seen = np.zeros(w * h, bool)
    with options(device, ACCEL=accel):
        for rank in range(3):
            stripes = dict(stripe_rows=4, n_ranks=3, rank=rank)
            gids = do.local_gids(w, h, **stripes)
            got = ls.gpu_render(device, tris, mats, est, cam, w, h, 1, **stripes)
            _compare(got, (wfb[gids], wws[:, gids]), "%s, rank %d" % (est.name, rank))
            counts, _ = _ao(device, tris, cam, w, h, 1, **stripes)
            assert np.array_equal(counts.reshape(-1, 2), wao[gids]), "AO counts, rank %d" % rank
            seen[gids] = True
    assert seen.all()


# ---- pt_camera_rays -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search,camera", [("lds", "reference"), ("lds", "oblique"), ("lbvh", "oblique")])
def test_camera_rays(device, search, camera):
    from oclpathtracer_amd.query import RayCaster

    tris, mats, accel = _scene(search)
    cam = ls.CAMERAS[camera]()
    frame = 3
    want = lo.camera_rays(cam, W, H, frame)
    with options(device, ACCEL=accel):
        rc = RayCaster(device, tris)
        try:
            rays = rc.camera_rays(W, H, frame, cam)
            got = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)
            assert_fb_equal(got[:, :7], want[:, :7], "origins, tmax and directions")
            assert len(np.unique(got[:, :3], axis=0)) > W * H // 2, "the origins coincide: no lens"
            hits = rc.closest(rays)
        finally:
            rc.release()
    gid = np.arange(W * H, dtype=np.int32)
    with lo.lens(*lo.lens_of(cam)):
        hit = do.decisions(tris, mats, W, H, gid, np.full(W * H, frame, np.int32), 1, cam=cam)[0]
    assert np.array_equal(hits["tri"] >= 0, hit.astype(bool)), "the query of the lens rays and the lens render's primary hits differ"
    assert 0 < hit.sum()


# ---- pinhole identities, GPU against GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search", ["lds", "lbvh"])
def test_pinhole_identity(device, search):
    """lens_radius = 0 with focus_distance = 7.5 is the camera without a lens, in workspace and framebuffer"""
    tris, mats, accel = _scene(search)
    plain = Camera(**ls.OBLIQUE)
    zero = plain.with_lens(0.0, 7.5)
    assert zero.focus_distance == 7.5
    rr_mis = ls.Estimator("indirect_rr_mis", True, dict(mis=True, roulette=ls.RR))
    with options(device, ACCEL=accel):
        for est in (ls.BY_NAME["direct_power"], rr_mis):
            a = ls.gpu_render(device, tris, mats, est, plain, W, H, FRAMES)
            b = ls.gpu_render(device, tris, mats, est, zero, W, H, FRAMES)
            assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes(), est.name
        ca, ia = _ao(device, tris, plain, W, H, FRAMES)
        cb, ib = _ao(device, tris, zero, W, H, FRAMES)
        assert ca.tobytes() == cb.tobytes() and ia.tobytes() == ib.tobytes(), "AO"
    assert np.array_equal(ca, ao_oracle.counts(tris, W, H, 0, FRAMES, 4, 1.5, cam=plain)), "and both are the pinhole's"


# ---- a wild lens: wider than the room, focused half a unit ahead -----------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
def test_wild_lens(device, accel):
    tris, mats = scene.load_model()
    cam = ls.reference_lens(3.0, 0.5)
    with options(device, ACCEL=accel):
        for name in ("direct_power", "indirect_rr"):
            est = ls.BY_NAME[name]
            want = ls.oracle_render(tris, mats, est, cam, W, H, FRAMES)
            _compare(ls.gpu_render(device, tris, mats, est, cam, W, H, FRAMES), want, "%s, R = 3, F = 0.5, accel %d" % (name, accel))
        counts, _ = _ao(device, tris, cam, W, H, FRAMES)
        assert np.array_equal(counts, ls.ao_counts(tris, cam, W, H, 0, FRAMES, 4, 1.5))
        # a search cut short would be reported by the next call (PT_ERR_TRAVERSAL is deferred): none is
        _ao(device, tris, None, 4, 4, 1)


# ---- autofocus --------------------------------------------------------------------------------------------------------------------------------
def test_autofocus(device):
    from oclpathtracer_amd.query import RayCaster

    tris, _ = scene.load_model()
    ref = Camera.reference()
    rc = RayCaster(device, tris)
    try:
        # image position (0.5, 0.05): the ray (0, 0.9 tan 30, -1) from y = 2.75 meets the ceiling y = 5.488 at t = 2.738 sqrt(1.27 / 0.27)
        up = ref.autofocus(rc, 0.05, 0.5, 0.05)
        assert up.lens_radius == float(np.float32(0.05))
        assert abs(up.focus_distance - 2.738 * math.sqrt(1.27 / 0.27)) < 2e-6 * up.focus_distance
        # the centre ray of a camera at (0, 2.75, 4) looking down -x from outside the open front: past the room, nothing
        with pytest.raises(ValueError):
            Camera((0.0, 2.75, 4.0), (-1.0, 2.75, 4.0)).autofocus(rc, 0.05)
        # a camera above the floor looking straight down: the floor y = 0 at t = 1.5, whatever the image's shape
        down = Camera((-2.0, 1.5, -0.5), (-2.0, 0.0, -0.5), up=(0.0, 0.0, -1.0))
        assert abs(down.autofocus(rc, 0.1, aspect=2.0).focus_distance - 1.5) < 1e-6
    finally:
        rc.release()
    on = ref.with_lens(0.05, focus_on=(0.0, 5.488, 4.0 - 2.738 / (0.9 * math.tan(math.radians(30.0)))))
    assert abs(on.focus_distance - up.focus_distance) < 2e-6 * up.focus_distance, "focus_on the same point"


# ---- errors through the C ABI -------------------------------------------------------------------------------------------------------------------
BAD_LENSES = [(-1.0, 4.0, None), (float("nan"), 4.0, None), (float("inf"), 4.0, None), (0.1, -1.0, None), (0.0, float("nan"), None),
              (0.1, float("inf"), None), (0.1, 0.0, None), (0.0, 0.0, 2), (0.0, 0.0, 3), (0.0, 0.0, 4), (0.0, 0.0, 5)]


def _bad_cameras():
    for R, F, reserved in BAD_LENSES:
        c = shim.Camera()
        shim.load().pt_camera_reference(ctypes.byref(c))
        c.lens_radius, c.focus_distance = R, F
        if reserved is not None:
            c.reserved[reserved] = 1
        yield (R, F, reserved), c


def test_bad_lenses_are_refused_and_nothing_is_written(device):
    tris, mats = scene.load_model()
    lib = shim.load()
    w, h = 8, 8
    d = LitBuffers("pt_render_direct", device, tris, mats, w, h)
    r = PixelBuffers(device, (tris, mats, None, None), w, h)
    a = ao_mod.AORenderer(device, tris, w, h, rays_per_sample=2)
    rays = adl.Buffer(device, w * h * 32, np.uint8)
    try:
        sent8 = np.full(w * h * 32, 0xa5, np.uint8)
        rays.write(sent8, sent8.size)
        sent_counts = np.full((h, w, 2), 0xdeadbeef, np.uint32)
        a.counts.write(sent_counts, sent_counts.size)
        sent_image = np.full((w * h, 4), np.float32(-7.25), np.float32)
        a.image.write(sent_image, w * h)
        for what, c in _bad_cameras():
            cam = ctypes.byref(c)
            assert d.call(d.params(2), cam=cam) == shim.PT_ERR_INVALID, what
            assert r.rr(r.params(r.nl), cam=cam) == shim.PT_ERR_INVALID, what
            p = a.params(1, 0)
            assert lib.pt_render_ao(device._h, a.tbuf._h, a.counts._h, a.image._h, ctypes.byref(p), cam, None) == shim.PT_ERR_INVALID, what
            assert lib.pt_camera_rays(device._h, cam, w, h, 0, rays._h, None) == shim.PT_ERR_INVALID, what
        d.assert_untouched()
        r.assert_untouched()
        assert np.array_equal(r.workspace(), r.ws_sentinel), "the workspace was written"
        assert np.array_equal(a.read_counts(), sent_counts) and np.array_equal(a.read_image(), sent_image), "AO buffers were written"
        out = np.zeros_like(sent8)
        rays.read(out, out.size)
        device.waitForCompletion()
        assert np.array_equal(out, sent8), "the ray buffer was written"
    finally:
        for b in (d, r, a, rays):
            b.release()


def test_the_fused_renderers_refuse_a_lens(device):
    from oclpathtracer_amd.distributed import StripeImage
    from oclpathtracer_amd.indirect import IndirectRenderer
    from oclpathtracer_amd.progressive import ProgressiveRenderer
    from oclpathtracer_amd.render import Renderer

    tris, mats = scene.load_model()
    lens, plain = ls.oblique_lens(), Camera(**ls.OBLIQUE)
    w, h, frames = 16, 16, 2
    r = Renderer(device, tris, mats, w, h, camera=plain)
    try:
        sentinel = np.full((w * h, 4), np.float32(-7.25), np.float32)
        r.fb.write(sentinel, w * h)
        p = shim.RenderParams()
        p.width, p.height, p.frame_begin, p.frame_count, p.max_bounces = w, h, 0, frames, 4
        p.num_triangles, p.num_materials, p.stripe_rows, p.n_ranks, p.rank = len(tris), len(mats), 16, 1, 0
        s = lens.to_struct()
        rc = shim.load().pt_render_frames_camera(device._h, r.tbuf._h, r.mbuf._h, r.fb._h, ctypes.byref(p), ctypes.byref(s), None, None)
        assert rc == shim.PT_ERR_INVALID
        assert b"pt_render_indirect" in shim.load().pt_last_error(), "the message names the way round"
        assert_fb_equal(r.read(), sentinel, "framebuffer after the refused render")
        with pytest.raises(ValueError, match="IndirectRenderer"):
            r.set_camera(lens)
        assert r.camera is plain
        for make in (lambda: Renderer(device, tris, mats, w, h, camera=lens), lambda: ProgressiveRenderer(device, tris, mats, w, h, camera=lens),
                     lambda: StripeImage(device, tris, mats, w, h, camera=lens)):
            with pytest.raises(ValueError, match="IndirectRenderer"):
                make()
        # the same camera with the lens removed still renders -- and the way round renders that image bit for bit
        r.set_camera(lens.with_lens(0.0))
        r.render(frames, max_bounces=4)
        fused = r.read()
    finally:
        r.release()
    none = np.zeros(0, np.int32)
    way = IndirectRenderer(device, tris, mats, w, h, max_bounces=4, lights=none, camera=plain, chunk_frames=frames)
    try:
        way.render(frames)
        assert_fb_equal(way.read(), fused, "IndirectRenderer with no lights against the fused renderer")
        way.set_camera(lens)
        way.render(frames, 0)
        got = way.read()
    finally:
        way.release()
    with lo.lens(*lo.lens_of(lens)):
        import indirect_oracle
        want = indirect_oracle.render(tris, mats, w, h, 0, frames, 1, 4, lights=none, cam=lens)
    assert_fb_equal(got, want, "... which takes the lens")


# ---- the harness ----------------------------------------------------------------------------------------------------------------------------------
def test_harness_lens(device, tmp_path):
    """raytrace_test --lens R: focused where the image's centre ray hits (the tall block's face, 6.925 from the eye), one PPM named _lens"""
    out, name, px = harness_ppm(tmp_path, 32, 2, "IndirectIllumination", "--roulette", "3", "--lens", "0.2")
    assert name.endswith("_rr_lens.ppm"), name
    line = [ln for ln in out.split("\n") if ln.startswith("lens: ")]
    assert len(line) == 1 and line[0].startswith("lens: radius 0.2, focused at 6.925"), out
    assert px.min() >= 0 and px.max() <= 255 and px.std() > 0
