"""Every renderer at the ends of what the C ABI accepts -- images of 2^31 - 64 pixels, global rows and columns beyond the exact floats,
frame numbers up to 2^31 - 2 -- against the CPU oracle, bit for bit (assert_fb_equal: equal bits, equal NaN positions; no tolerance
anywhere).  The inputs and what the oracle says of them are tests/extent_cases.py's; tests/test_extents_cpu.py proves that each reaches
its corner.  A rank of a striped render owns a few rows however large the image, so every case but WIDE has a few hundred pixels.
The lit estimators include the RIS, environment and thin-lens forms; the pixel lists, the features, the lens AO render and the lens
rays are in tests/test_gpu_extents_lists.py.

WIDE, (2^24 + 256) x 127, is one row of 16 777 472 pixels, 134 M samples all but a few thousand of which miss the scene; its renders
go through a device handle of their own, so that the 0.5 GB staging ring it needs does not change the chunking of the tests after it.
Under PT_OPT_PRIMARY_MASKS 1 a table made there drops triangles the reference hits (the footprint bound's premise fails from column
2^23 on; measured on an MI355X before the host's decision existed: 3 of the window's 257 pixels lost an accepted triangle and differed
from the oracle's after 8 frames); the host declines the masks for such an image (pmask_footprint_holds, pt_shim.hip), and a test here
pins that decision at its threshold.  frame_begin = 2^31 - 4 is what found the fold kernel's reciprocal-table loop starting at
frame_begin + threadIdx.x, past 2^31 - 1: NaN pixels from every renderer (pt_fold_kernel clamps its start now)."""
import ctypes

import numpy as np
import pytest

import ao_oracle
import direct_oracle as do
import extent_cases as xc
import extent_oracle as eo
import primary_accept
from conftest import assert_fb_equal
from env_scenes import env_map
from gpu_support import lit_with_samples, options, render
from oclpathtracer_amd import adl, shim
from oclpathtracer_amd.ao import AORenderer
from oclpathtracer_amd.direct import DirectRenderer
from oclpathtracer_amd.environment import Environment
from oclpathtracer_amd.features import FeatureRenderer
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette
from oclpathtracer_amd.render import Renderer
from roulette_support import roulette_with_samples

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)


# ---- the fused renderer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("name", list(xc.TALL))
def test_fused_tall(device, name, accel):
    """three frames in three checkpointed launches: pixels, rays and samples are the oracle's at global rows up to 2^25 - 2"""
    tris, mats = xc.cornell()[:2]
    want, want_st = xc.fused_tall(name)
    with options(device, ACCEL=accel, CHECKPOINT=1, CHUNK_FRAMES=1):
        got, st = render(device, tris, mats, xc.TALL_W, xc.TALL_H, xc.TALL_FRAMES, want_stats=True, **xc.TALL[name])
    assert len(got) == xc.TALL_ROWS[name] * xc.TALL_W
    assert_fb_equal(got, want, "%s accel %d" % (name, accel))
    assert int(st[shim.PT_STAT_RAYS]) == int(want_st[0]), "%d rays, the oracle traced %d" % (int(st[shim.PT_STAT_RAYS]), int(want_st[0]))
    assert int(st[shim.PT_STAT_SAMPLES]) == int(want_st[1])


@pytest.mark.parametrize("name,chunk", [("table_end", 0), ("table_end", 2), ("float_ties", 0), ("last_frames", 0)])
def test_fused_late(device, name, chunk):
    """resumed from arbitrary pixels at late frames; at z = 2046 .. 2050 with chunks of 2 the end of the fold's reciprocal table falls
    between two fold launches, with one chunk inside a launch"""
    tris, mats = xc.cornell()[:2]
    frame_begin, frames = xc.LATE[name]
    want, want_st = xc.fused_late(name)
    with options(device, CHUNK_FRAMES=chunk):
        got, st = render(device, tris, mats, xc.LATE_W, xc.LATE_H, frames, frame_begin=frame_begin, fb_init=xc.late_start(),
                         want_stats=True, stripe_rows=1)
    assert_fb_equal(got, want, "%s, frames from %d, chunks of %d" % (name, frame_begin, chunk))
    assert int(st[shim.PT_STAT_RAYS]) == int(want_st[0]) and int(st[shim.PT_STAT_SAMPLES]) == int(want_st[1])


def test_one_frame_beyond_the_last_is_refused(device):
    tris, mats = xc.cornell()[:2]
    start = xc.late_start()
    r = Renderer(device, tris, mats, xc.LATE_W, xc.LATE_H, stripe_rows=1)
    try:
        r.fb.write(start, r.local_pixels)
        with pytest.raises(shim.ShimError) as e:
            r.render(4, frame_begin=2 ** 31 - 4)          # frame_begin + frame_count = 2^31
        assert e.value.code == shim.PT_ERR_INVALID
        assert np.array_equal(r.read(), start), "the framebuffer was touched"
    finally:
        r.release()


@pytest.fixture(scope="module")
def wide_device():
    """a handle of its own for the WIDE renders: their staging ring and mask table go with it"""
    dev = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    yield dev
    adl.DeviceUtils.deallocate(dev)


def _read_columns(r, blocks, scattered):
    """the pixels of the column blocks, then of the single columns, of a one-row framebuffer: only what is compared is read back"""
    out = np.zeros((sum(n for _, _, n in blocks) + len(scattered), 4), np.float32)
    k = 0
    for _, first, n in blocks:
        r.fb.read(out[k: k + n], n, first)
        k += n
    for c in scattered:
        r.fb.read(out[k: k + 1], 1, int(c))
        k += 1
    r.dev.waitForCompletion()
    return out


def _mask_snapshot(dev, expect_pixels):
    """None when no table stands (the host declined the masks); else the table, which must be this render's"""
    lib = shim.load()
    n = ctypes.c_uint32(0)
    rc = lib.pt_primary_mask_snapshot(dev._h, ctypes.byref(n), None, 0)
    if rc == shim.PT_ERR_INVALID:
        return None
    shim.check(rc)
    assert n.value == expect_pixels, "the table stands for %d pixels, the render has %d" % (n.value, expect_pixels)
    out = np.zeros((n.value, 2), np.uint32)
    shim.check(lib.pt_primary_mask_snapshot(dev._h, ctypes.byref(n), out.ctypes.data_as(ctypes.c_void_p), len(out)))
    return out


@pytest.mark.parametrize("masks", [0, 1])
def test_fused_wide(wide_device, masks):
    """masks 0: the column walk and the seeds at W = 2^24 + 256.  masks 1: the same pixels -- and if a table stands for the render, it
    keeps every triangle the reference accepts over 32 frames at the window's pixels"""
    dev = wide_device
    tris, mats = xc.cornell()[:2]
    blocks, scattered = xc.wide_columns()
    want, want_st = xc.fused_wide()
    with options(dev, ACCEL=1, PRIMARY_MASKS=masks):
        r = Renderer(dev, tris, mats, xc.WIDE_W, xc.WIDE_H, **xc.WIDE_STRIPES)
        try:
            assert r.local_pixels == xc.WIDE_W
            r.render(xc.WIDE_FRAMES)
            got = _read_columns(r, blocks, scattered)
            snap = _mask_snapshot(dev, r.local_pixels) if masks else None
        finally:
            r.release()
    if snap is not None:
        cols = xc.window_columns()
        acc, _, _, _ = primary_accept.union(tris, xc.WIDE_W, xc.WIDE_H, xc.WIDE_MASK_FRAMES, gid=xc.wide_gids(cols))
        lost = acc & ~primary_accept.mask_bits(snap[cols], len(tris))
        print("masks were made: %d of the window's %d pixels lost an accepted triangle" % (int((lost != 0).sum()), len(cols)))
    else:
        lost = np.zeros(1, np.uint64)
        print("no mask table stands for the render" if masks else "masks off")
    k = 0
    for name, _, n in blocks + [("scattered", 0, len(scattered))]:
        g, w = got[k: k + n], want[k: k + n]
        bad = int((g.view(np.uint32) != w.view(np.uint32)).any(axis=1).sum())
        print("%s: %d of %d pixels differ from the oracle's" % (name, bad, n))
        k += n
    k = 0
    for name, _, n in blocks + [("scattered", 0, len(scattered))]:
        assert_fb_equal(got[k: k + n], want[k: k + n], "masks %d, %s columns" % (masks, name))
        k += n
    assert not lost.any(), "%d pixels of the window lost an accepted triangle" % int((lost != 0).sum())


def _window(W, n=129):
    first = max(0, W // 2 - n // 2)
    return np.arange(first, min(W, first + n), dtype=np.int64)


@pytest.mark.parametrize("W,H,stripes,stands", [
    (4096, 4096, dict(stripe_rows=1, n_ranks=2048, rank=1023), True),     # the largest image every benchmark configuration stays within
    (7625, 123, dict(stripe_rows=1, n_ranks=123, rank=61), True),         # 7625^2 + 123^2 = 58 155 754 <= 7626^2 = 58 155 876
    (123, 7625, dict(stripe_rows=1, n_ranks=1525, rank=762), True),
    (5392, 5392, dict(stripe_rows=1, n_ranks=2696, rank=1347), True),     # 2 * 5392^2 = 58 147 328
    (7625, 124, dict(stripe_rows=1, n_ranks=124, rank=62), False),        # 7625^2 + 124^2 = 58 156 001: declined
    (5393, 5393, dict(stripe_rows=1, n_ranks=2696, rank=1348), False),
], ids=lambda v: None if isinstance(v, (dict, bool)) else str(v))
def test_masks_are_declined_only_beyond_the_footprint_bound(device, W, H, stripes, stands):
    """the host's decision (pmask_footprint_holds, width^2 + height^2 <= 7626^2) at its threshold, on renders of a few thousand pixels:
    where masks are made they keep what the reference accepts about the image's centre and the pixels are the oracle's; where they are
    declined no table stands and the pixels are the oracle's"""
    tris, mats = xc.cornell()[:2]
    assert (W * W + H * H <= 7626 * 7626) == stands
    with options(device, ACCEL=1, PRIMARY_MASKS=1):
        r = Renderer(device, tris, mats, W, H, **stripes)
        try:
            r.render(2)
            got = r.read()
            snap = _mask_snapshot(device, r.local_pixels)
            n = r.local_pixels
        finally:
            r.release()
    gids = do.local_gids(W, H, **stripes)
    assert len(gids) == n
    rows = np.unique(gids // W)
    pick = rows[len(rows) // 2] * W + _window(W)   # about the centre of the local row nearest the image's middle
    lp = np.searchsorted(gids, pick)
    want, _ = eo.render_window(tris, mats, W, H, 2, pick)
    assert_fb_equal(got[lp], want, "%d x %d" % (W, H))
    assert (snap is not None) == stands, "a mask table %s for %d x %d" % ("stands" if snap is not None else "does not stand", W, H)
    if stands:
        acc, _, _, _ = primary_accept.union(tris, W, H, xc.WIDE_MASK_FRAMES, gid=pick)
        assert acc.any(), "no primary ray of the picked pixels hits anything"
        lost = acc & ~primary_accept.mask_bits(snap[lp], len(tris))
        assert not lost.any(), "%d pixels lost an accepted triangle" % int((lost != 0).sum())


# ---- the lit renderers -------------------------------------------------------------------------------------------------------------
def _lit(device, est, tall, W, H, frames, **kw):
    """one render of an estimator of xc.LIT on its scene (xc.scene_of) through the entry point the Python renderers choose for it --
    pt_render_direct_ris / pt_render_indirect_ris with candidates, pt_render_direct_env / pt_render_indirect_env with the map, the camera
    with its lens: (framebuffer, the sample workspace)"""
    e = xc.LIT[est]
    sc = xc.scene_of(est, tall)
    if not (e.M or e.Ke or e.lens):   # what existed before, as before
        if e.rr is not None:
            return roulette_with_samples(device, sc, W, H, frames, xc.LIT_K, e.B, e.rr[0], e.rr[1], mis=e.mis, power=e.power, **kw)
        return lit_with_samples(device, sc, W, H, frames, xc.LIT_K, max_bounces=e.B, mis=e.mis, **kw)
    if e.M:
        kw["candidates"] = e.M
    if e.Ke:
        kw.update(environment=Environment(env_map(xc.ENV_MAP)), env_samples=e.Ke)
    if e.rr is not None:
        kw["roulette"] = Roulette(*e.rr)
    try:
        return lit_with_samples(device, sc, W, H, frames, xc.LIT_K, max_bounces=e.B, mis=e.mis, light_choice="power" if e.power else "uniform", **kw)
    finally:
        if e.Ke:
            kw["environment"].release()


@pytest.mark.parametrize("name", list(xc.TALL))
@pytest.mark.parametrize("est", list(xc.LIT))
def test_lit_tall(device, est, name):
    """TALL: gids up to W * H - 1 under every estimator -- RIS (4M - 1 uniforms per light sample), the environment, the lens (two more
    draws, a shifted origin)"""
    want_fb, want_ws = xc.lit_tall(est, name)
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            fb, ws = _lit(device, est, True, xc.TALL_W, xc.TALL_H, xc.LIT_FRAMES, **xc.TALL[name])
        assert_fb_equal(ws, want_ws, "%s %s accel %d: radiance before the fold" % (est, name, accel))
        assert_fb_equal(fb, want_fb, "%s %s accel %d" % (est, name, accel))


@pytest.mark.parametrize("name", list(xc.LATE))
@pytest.mark.parametrize("est", list(xc.LIT))
def test_lit_late(device, est, name):
    """LATE: frame numbers about 2048, 2^24 and up to 2^31 - 2 under every estimator"""
    frame_begin, frames = xc.LATE[name]
    want_fb, want_ws = xc.lit_late(est, name)
    fb, ws = _lit(device, est, False, xc.LATE_W, xc.LATE_H, frames, frame_begin=frame_begin, fb_init=xc.late_start())
    assert_fb_equal(ws, want_ws, "%s %s: radiance before the fold" % (est, name))
    assert_fb_equal(fb, want_fb, "%s %s" % (est, name))


# ---- ambient occlusion -------------------------------------------------------------------------------------------------------------
AO_RADIUS = 1.5


def _ao(device, tris, W, H, frames, K, frame_begin=0, start=None, **stripes):
    r = AORenderer(device, tris, W, H, rays_per_sample=K, radius=AO_RADIUS, **stripes)
    try:
        if start is not None:
            r.counts.write(np.ascontiguousarray(start, np.uint32), 2 * r.local_pixels)
        r.render(frames, frame_begin)
        return r.read_counts()
    finally:
        r.release()


@pytest.mark.parametrize("name", list(xc.TALL))
def test_ao_tall(device, name):
    tris = xc.cornell()[0]
    want = ao_oracle.counts(tris, xc.TALL_W, xc.TALL_H, 0, 2, 2, AO_RADIUS, **xc.TALL[name])
    assert want[..., 1].sum() > 0 and 0 < want[..., 0].sum() < 2 * want[..., 1].sum(), "every ray open, or none: nothing is compared"
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            got = _ao(device, tris, xc.TALL_W, xc.TALL_H, 2, 2, **xc.TALL[name])
        assert np.array_equal(got, want), "%s accel %d: %d counts differ" % (name, accel, int((got != want).sum()))


@pytest.mark.parametrize("K", [1, 2])
def test_ao_last_frames(device, K):
    """frames 2^31 - 4 .. 2^31 - 2 added to counts in hand.  (frame_begin + frame_count) K is 2^31 - 1 and 2^32 - 2: both within what
    the counts hold (pt_shim.h: PT_ERR_RANGE above 2^32 - 1)"""
    tris = xc.cornell()[0]
    frame_begin, frames = xc.LATE["last_frames"]
    start = np.random.default_rng(9).integers(0, 1000, (xc.LATE_H, xc.LATE_W, 2)).astype(np.uint32)
    want = ao_oracle.counts(tris, xc.LATE_W, xc.LATE_H, frame_begin, frames, K, AO_RADIUS, start=start)
    assert not np.array_equal(want, start)
    got = _ao(device, tris, xc.LATE_W, xc.LATE_H, frames, K, frame_begin=frame_begin, start=start, stripe_rows=1)
    assert np.array_equal(got, want), "%d counts differ" % int((got != want).sum())


def test_ao_counts_that_could_wrap_stay_refused(device):
    """at frame_begin = 2^31 - 4 with 3 frames, K = 3 is the first whose (frame_begin + frame_count) K exceeds 2^32 - 1: PT_ERR_RANGE,
    the counts untouched; one frame more is PT_ERR_INVALID whatever K"""
    tris = xc.cornell()[0]
    frame_begin, frames = xc.LATE["last_frames"]
    lib = shim.load()
    r = AORenderer(device, tris, xc.LATE_W, xc.LATE_H, rays_per_sample=3, radius=AO_RADIUS, stripe_rows=1)
    try:
        start = np.full((r.local_pixels, 2), 0xA5A5A5A5, np.uint32)
        r.counts.write(start, 2 * r.local_pixels)

        def call(p):
            return lib.pt_render_ao(device._h, r.tbuf._h, r.counts._h, r.image._h, ctypes.byref(p), None, None)
        for K in (3, 256):
            p = r.params(frames, frame_begin)
            p.rays_per_sample = K
            assert call(p) == shim.PT_ERR_RANGE, "K = %d" % K
        p = r.params(frames + 1, frame_begin)
        p.rays_per_sample = 1
        assert call(p) == shim.PT_ERR_INVALID
        assert np.array_equal(r.read_counts().reshape(-1, 2), start), "the counts were touched"
    finally:
        r.release()


# ---- a rank without rows -----------------------------------------------------------------------------------------------------------
def _raw(device, buf, elements, dtype):
    """the first ``elements`` elements of a buffer as a flat array of ``dtype``"""
    out = np.zeros(elements * buf._dtype.itemsize // np.dtype(dtype).itemsize, dtype)
    buf.read(out, elements)
    device.waitForCompletion()
    return out


def test_a_rank_without_rows_renders_nothing(device):
    """EMPTY: H = 5 in stripes of 4 over 3 ranks: rank 2 owns no row.  Every entry point returns PT_OK (the wrappers raise otherwise),
    leaves its one-element buffers as they were and enqueues nothing that the following wait reports: the fused and the lit renderers,
    their RIS and environment forms, the features, ambient occlusion, the list renders of no slot, the moments of no pixel;
    pt_adaptive_select of no pixel writes a header of zeros"""
    tris, mats, lights, cam = xc.cornell()
    W, H, st = xc.EMPTY_W, xc.EMPTY_H, xc.EMPTY_STRIPES
    four = np.full((1, 4), SENTINEL, np.float32)
    lib = shim.load()
    sky = Environment(env_map(xc.ENV_MAP))
    r = Renderer(device, tris, mats, W, H, want_stats=True, **st)
    try:
        assert r.local_pixels == 0
        r.fb.write(four, 1)
        r.render(3)
        r.render(2, frame_begin=2 ** 31 - 3)
        assert np.array_equal(_raw(device, r.fb, 1, np.float32), four.reshape(-1))
        device.waitForCompletion()
        assert not r.read_stats_raw()[[shim.PT_STAT_RAYS, shim.PT_STAT_SAMPLES]].any()
    finally:
        r.release()
    lit = [DirectRenderer(device, tris, mats, W, H, light_samples=1, chunk_frames=2, **st),
           IndirectRenderer(device, tris, mats, W, H, light_samples=1, max_bounces=4, chunk_frames=2, **st),
           IndirectRenderer(device, tris, mats, W, H, light_samples=1, max_bounces=4, mis=True, light_choice="power", roulette=Roulette(1, 0.5),
                            chunk_frames=2, **st),
           DirectRenderer(device, tris, mats, W, H, light_samples=1, chunk_frames=2, light_choice="power", candidates=xc.LIT_M, **st),
           IndirectRenderer(device, tris, mats, W, H, light_samples=1, max_bounces=4, mis=True, light_choice="power", roulette=Roulette(1, 0.5),
                            candidates=xc.LIT_M, chunk_frames=2, **st),
           DirectRenderer(device, tris, mats, W, H, light_samples=1, chunk_frames=2, light_choice="power", environment=sky,
                          env_samples=xc.LIT_KE, **st),
           IndirectRenderer(device, tris, mats, W, H, light_samples=1, max_bounces=4, mis=True, light_choice="power", roulette=Roulette(1, 0.5),
                            environment=sky, env_samples=xc.LIT_KE, chunk_frames=2, **st)]
    record = np.full(56, 0xA5, np.uint8)
    mb, pl = adl.Buffer(device, 56, np.uint8), adl.Buffer(device, lib.pt_adaptive_list_bytes(0), np.uint8)
    header = np.full(pl.getSize(), 0xA5, np.uint8)
    mb.write(record, 56)
    pl.write(header, len(header))
    for d in lit:
        try:
            what = "%s, %d candidates, %d environment samples" % (type(d).__name__, d.candidates, d.env_samples)
            assert d.local_pixels == 0
            d.fb.write(four, 1)
            ws = np.full(d.samples.getSize(), SENTINEL, np.float32)
            d.samples.write(ws, len(ws))
            d.render(3)
            d.render(2, 2 ** 31 - 3)
            if isinstance(d, IndirectRenderer) and d.roulette is not None and d.environment is None:
                # the list renders of no slot, through the plain and the RIS form, and the moments of no listed pixel
                head = (device._h, d.tbuf._h, d.mbuf._h, d._lights_h(), *d._estimator(), d.samples._h, d.fb._h, pl._h, 0,
                        ctypes.byref(d.params(3, 0)), ctypes.byref(d._rr))
                assert lib.pt_render_indirect_pixels(*head, None, None) == shim.PT_OK, what
                assert lib.pt_render_indirect_pixels_ris(*head, ctypes.byref(shim.Ris(xc.LIT_M)), None, None) == shim.PT_OK, what
                assert lib.pt_sample_moments_pixels(device._h, d.samples._h, mb._h, pl._h, 0, 3, None) == shim.PT_OK, what
                assert lib.pt_sample_moments(device._h, d.samples._h, mb._h, 0, 3, 1, None) == shim.PT_OK, what
            assert np.array_equal(_raw(device, d.fb, 1, np.float32), four.reshape(-1)), what
            assert np.array_equal(_raw(device, d.samples, len(ws), np.float32), ws), what
            assert np.array_equal(_raw(device, mb, 56, np.uint8), record) and np.array_equal(_raw(device, pl, len(header), np.uint8), header), what
            device.waitForCompletion()
        finally:
            d.release()
    sky.release()
    # selection and resolve of no pixel
    nb, sb = adl.Buffer(device, 16, np.uint8), adl.Buffer(device, max(48, lib.pt_moments_summary_bytes(0)), np.uint8)
    try:
        noise = np.full(16, 0xA5, np.uint8)
        summary = np.full(sb.getSize(), 0xA5, np.uint8)
        nb.write(noise, 16)
        sb.write(summary, len(summary))
        assert lib.pt_moments_resolve(device._h, mb._h, 0, nb._h, sb._h, None) == shim.PT_OK
        assert np.array_equal(_raw(device, nb, 16, np.uint8), noise) and np.array_equal(_raw(device, sb, len(summary), np.uint8), summary)
        rule = shim.AdaptiveRule(0.0, 0.0, 1, 1)
        assert lib.pt_adaptive_select(device._h, mb._h, 0, ctypes.byref(rule), pl._h, None) == shim.PT_OK
        assert not _raw(device, pl, 16, np.uint8).any(), "the header of an empty selection is not zeros"
        assert np.array_equal(_raw(device, mb, 56, np.uint8), record)
        device.waitForCompletion()
    finally:
        for b in (mb, pl, nb, sb):
            b.release()
    # the features
    f = FeatureRenderer(device, tris, mats, W, H, features=("albedo", "normal", "depth", "emission"), workspace_frames=3, **st)
    try:
        assert f.local_pixels == 0
        ws = np.full(9, SENTINEL, np.float32)
        for name in f.features:
            f.samples[name].write(ws, 9)
            f.mom[name].write(record, 56)
        f.render(3)
        p = f.params(2, 2 ** 31 - 3)
        assert lib.pt_render_features(device._h, f.tbuf._h, f.mbuf._h, *[f.samples[n]._h for n in f.features], ctypes.byref(p), None, None) == shim.PT_OK
        for name in f.features:
            assert np.array_equal(_raw(device, f.samples[name], 9, np.float32), ws), name
            assert np.array_equal(_raw(device, f.mom[name], 56, np.uint8), record), name
        device.waitForCompletion()
    finally:
        f.release()
    a = AORenderer(device, tris, W, H, rays_per_sample=2, radius=AO_RADIUS, **st)
    try:
        assert a.local_pixels == 0
        two = np.full(2, 0xA5A5A5A5, np.uint32)
        a.counts.write(two, 2)
        a.image.write(four, 1)
        a.render(3)
        assert np.array_equal(_raw(device, a.counts, 2, np.uint32), two) and np.array_equal(_raw(device, a.image, 1, np.float32), four.reshape(-1))
        device.waitForCompletion()
    finally:
        a.release()
