"""The bounce loop's state (GPU tier): the table trace kernels keep "which lanes hold a live path" as one wave-uniform lane mask, changed
where paths park, resume, start and finish, and shading reports "finished" instead of clearing a per-lane flag; their pass-1 filter no
longer tests the length of a direction the kernel itself normalised.

Every render is compared bit for bit with the CPU oracle, ray and sample counts included.  The shapes are the smallest at which a lane
mask or a changed shade exit can go wrong: partial waves, fewer samples than one wave, paths that all end at once or in their first
shading, waves that resume parked paths across launches, local pixels that are not global ones, every pass-1 form.  The query kernel
kept the direction test: rays that are far from unit length go through it against the query oracle.
"""
import numpy as np
import pytest

import query_oracle as qo
import scenes
from conftest import assert_fb_equal
from gpu_support import assert_hits_equal, cornell_rays, options, render
from oclpathtracer_amd import shim

pytestmark = pytest.mark.gpu

FRAMES = 3


def _assert_render(device, tris, mats, w, h, frames, oracle, what, depth=16, want=None):
    """One render against the oracle: pixels, rays and samples.  ``want``: the oracle's (image, tallies) when the caller shares them."""
    fb, ost = want if want is not None else oracle.render(tris, mats, w, h, frames, max_bounces=depth, want_stats=True)
    got, st = render(device, tris, mats, w, h, frames, depth=depth, want_stats=True)
    assert_fb_equal(got, fb, what)
    assert int(st[shim.PT_STAT_RAYS]) == ost["rays"], "%s: %d rays, the oracle traced %d" % (what, int(st[shim.PT_STAT_RAYS]), ost["rays"])
    assert int(st[shim.PT_STAT_SAMPLES]) == ost["samples"] == w * h * frames, what
    return ost


@pytest.fixture(scope="module")
def cornell_64x64_f5(cornell, oracle):
    """The oracle's 64 x 64 image after 5 frames and its tallies: computed once, shared, never written."""
    tris, mats = cornell
    fb, st = oracle.render(tris, mats, 64, 64, 5, want_stats=True)
    fb.setflags(write=False)
    return fb, st


@pytest.mark.parametrize("w,h", [(33, 97), (5, 3)])
@pytest.mark.parametrize("depth", [1, 16])
def test_partial_waves_and_both_path_lengths(device, cornell, oracle, w, h, depth):
    """33 x 97: rows shorter than a wave, a ragged last wave.  5 x 3: fewer samples than one wave holds lanes, so most of the mask is
    never set.  Depth 1: every path ends in its first shading (the whole mask clears at once, bounce after bounce); depth 16: paths end a
    few per bounce and the freed lanes take parked ones."""
    tris, mats = cornell
    _assert_render(device, tris, mats, w, h, FRAMES, oracle, "%d x %d, depth %d" % (w, h, depth), depth=depth)


def test_every_primary_ray_misses(device, cornell, oracle):
    """The box moved a thousand units aside: every sample ends at its first ray, all lanes of a wave finish together and a wave leaves
    the loop with an empty mask."""
    tris, mats = cornell
    away = tris.copy()
    for f in ("p1", "p2", "p3"):
        away[f][:, 0] += np.float32(1000.0)
    w, h = 33, 17
    ost = _assert_render(device, away, mats, w, h, FRAMES, oracle, "nothing in view")
    assert ost["rays"] == w * h * FRAMES, "the scene is in view after all"


def test_one_material_id_out_of_range(device, oracle):
    """One triangle with an id beyond the materials: shading clamps it, and the path goes on or ends as the clamped material says."""
    tris, mats = scenes.variant("quads_scaled")
    bad = tris.copy()
    bad["id"][0] = len(mats) + 1000
    clamped = bad.copy()
    clamped["id"] = np.clip(bad["id"], 0, len(mats) - 1)
    w, h = 48, 40
    want = oracle.render(clamped, mats, w, h, FRAMES, want_stats=True)
    assert not np.array_equal(want[0], oracle.render(tris, mats, w, h, FRAMES)), "the corrupt triangle is not in view"
    _assert_render(device, bad, mats, w, h, FRAMES, oracle, "a material id out of range", want=want)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("checkpoint", [1, 0])
def test_one_frame_chunks(device, cornell, cornell_64x64_f5, checkpoint, lanes):
    """64 x 64, five launches of one frame each.  Checkpointed, a wave parks its live paths at the end of a launch and the next launch's
    wave resumes them into lanes 0 .. n - 1: the mask is rebuilt from the region's count."""
    tris, mats = cornell
    with options(device, CHUNK_FRAMES=1, CHECKPOINT=checkpoint, RENDER_LANES=lanes):
        got, st = render(device, tris, mats, 64, 64, 5, want_stats=True)
    what = "one-frame chunks, checkpoint %d, lanes %d" % (checkpoint, lanes)
    fb, ost = cornell_64x64_f5
    assert_fb_equal(got, fb, what)
    assert int(st[shim.PT_STAT_RAYS]) == ost["rays"] and int(st[shim.PT_STAT_SAMPLES]) == 64 * 64 * 5, what
    if checkpoint:
        assert int(st[shim.PT_STAT_CARRIED]) > 0, "no path crossed a launch boundary"


def test_two_rank_stripes_on_one_device(device, cornell, oracle):
    """Both ranks of a two-rank split with 4-row stripes, one after the other on the one device: 33 x 22 leaves rank 1 a ragged last
    stripe, and a fresh wave's 64 samples span two rows of which the second may lie in another stripe."""
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    w, h = 33, 22
    want, ost = oracle.render(tris, mats, w, h, FRAMES, want_stats=True)
    want = want.reshape(h, w, 4)
    rays = samples = 0
    for rank in (0, 1):
        r = Renderer(device, tris, mats, w, h, n_ranks=2, rank=rank, stripe_rows=4, want_stats=True)
        try:
            r.render(FRAMES)
            got, rows, st = r.read(), r.global_rows(), r.read_stats()
        finally:
            r.release()
        assert_fb_equal(got, want[rows].reshape(-1, 4), "rank %d of 2, 4-row stripes" % rank)
        rays, samples = rays + st["rays"], samples + st["samples"]
    assert rays == ost["rays"] and samples == w * h * FRAMES


@pytest.mark.parametrize("quad", [0, 1, 4])
def test_every_pass1_form(device, cornell, oracle, quad):
    """PT_OPT_QUAD_FILTER 0, 1 and 4: the independent-triangle filter and the shared-u forms (the packed one no longer tests |d|^2)."""
    tris, mats = cornell
    w, h = 33, 17
    with options(device, QUAD_FILTER=quad):
        _assert_render(device, tris, mats, w, h, FRAMES, oracle, "PT_OPT_QUAD_FILTER %d" % quad)


def test_queries_keep_the_direction_test(device, cornell):
    """Closest hits of rays whose directions have length 3: the query kernel takes callers' rays, so its filter still tests |d|^2 and
    falls back to the exact test for these."""
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(5), 4096, tris)
    d = rays[:, 4:7].astype(np.float64)
    n = np.sqrt((d * d).sum(1, keepdims=True))
    ok = n[:, 0] > 0
    rays[ok, 4:7] = (3.0 * d[ok] / n[ok]).astype(np.float32)
    want = qo.closest(tris, rays)
    assert (want[:, 1].view(np.int32) >= 0).mean() > 0.3
    rc = RayCaster(device, tris)
    try:
        got = rc.closest(rays)
    finally:
        rc.release()
    assert_hits_equal(got, want, "directions of length 3")
