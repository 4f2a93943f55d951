"""Where a finished path's radiance goes (GPU tier): a path carries the position of its record in the staging ring -- worked out once,
where its sample starts -- instead of its local pixel, and shading gathers the hit's normal and material by 32-bit offsets.

Every case is compared bit for bit with the CPU oracle.  The shapes are the smallest at which the address can still go wrong: a ring
that wraps and starts in its other slot, paths that cross launches, local pixels that are not global ones, the kernels that share
``pt_shade``, record offsets above 2^31 bytes and a ring too large for the 32-bit form, and the two gathers' edge cases.
"""
from contextlib import contextmanager

import numpy as np
import pytest

import scenes
from conftest import assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import adl, shim

pytestmark = pytest.mark.gpu

MIB = 1 << 20
W, H = 33, 97            # an odd width: rows straddle waves, the last wave of a frame is ragged
FIRST, SECOND = 13, 4    # frames of the first call and of the second, on the same framebuffer


@contextmanager
def _fresh_device(staging_bytes=2 * MIB):
    """A device handle of its own: its chunk sequence starts at 0, so which ring slot a render starts in is known."""
    dev = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    try:
        dev.reserveStaging(staging_bytes)
        yield dev
    finally:
        adl.DeviceUtils.deallocate(dev)


@pytest.fixture(scope="module")
def cornell_33x97(cornell, oracle):
    """The oracle's 33 x 97 images after 7, 13 and 17 frames: computed once, shared, never written."""
    tris, mats = cornell
    want = {n: oracle.render(tris, mats, W, H, n) for n in (7, FIRST, FIRST + SECOND)}
    for a in want.values():
        a.setflags(write=False)
    return want


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("checkpoint", [1, 0])
def test_ring_wrap_and_phase(cornell, cornell_33x97, checkpoint, lanes):
    """Chunks of three frames.  13 frames are more than the ring's 2S = 6 and no multiple of S, and they go as FIVE chunks (3, 3, 3, 3, 1):
    on a fresh handle the second call -- frames 13..16 on the same framebuffer, two chunks of two -- therefore starts in the OTHER slot
    (ring_phase = S != 0), with another S than the first call's."""
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    with _fresh_device() as dev, options(dev, CHUNK_FRAMES=3, CHECKPOINT=checkpoint, RENDER_LANES=lanes):
        r = Renderer(dev, tris, mats, W, H, want_stats=True)
        try:
            r.render(FIRST)
            first = r.read()
            r.render(SECOND)                      # continues at frame 13
            both = r.read()
            st = r.read_stats_raw()
        finally:
            r.release()
    what = "checkpoint %d, lanes %d" % (checkpoint, lanes)
    assert_fb_equal(first, cornell_33x97[FIRST], "13 frames in five chunks, " + what)
    assert_fb_equal(both, cornell_33x97[FIRST + SECOND], "then frames 13..16 from the other slot, " + what)
    assert int(st[shim.PT_STAT_SAMPLES]) == W * H * (FIRST + SECOND), what


def test_a_carried_path_keeps_its_address(device, cornell, cornell_33x97):
    """One-frame chunks at depth 16: every launch hands paths to the next, and each still stores to its own frame's record."""
    tris, mats = cornell
    with options(device, CHUNK_FRAMES=1):
        got, st = render(device, tris, mats, W, H, FIRST, depth=16, want_stats=True)
    assert int(st[shim.PT_STAT_CARRIED]) > 0, "no path crossed a launch boundary"
    assert_fb_equal(got, cornell_33x97[FIRST], "13 one-frame chunks")


def test_local_pixels_are_not_global_pixels(device, cornell, oracle):
    """Rank 1 of 3 with 4-row stripes of a 40 x 50 image (global rows 4..7, 16..19, 28..31, 40..43), two chunks: the record's position
    counts LOCAL pixels, the seed GLOBAL ones."""
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    w, h, frames = 40, 50, 5
    want = oracle.render(tris, mats, w, h, frames).reshape(h, w, 4)
    with options(device, CHUNK_FRAMES=3):
        r = Renderer(device, tris, mats, w, h, n_ranks=3, rank=1, stripe_rows=4)
        try:
            r.render(frames)
            got = r.read()
            rows = r.global_rows()
        finally:
            r.release()
    assert list(rows[:5]) == [4, 5, 6, 7, 16] and got.shape == (len(rows) * w, 4)
    assert_fb_equal(got, want[rows].reshape(-1, 4), "rank 1 of 3, 4-row stripes, chunks of 3 + 2 frames")


@pytest.mark.parametrize("accel", [2, 1])
def test_lbvh_and_tiled_kernels_share_the_store(device, cornell, oracle, accel):
    """600 triangles through the LBVH kernel (PT_OPT_ACCEL 2) and the tiled brute-force kernel (1), 7 frames in chunks of two."""
    tris, mats = scenes.soup(600), cornell[1]
    w, h, frames = 64, 48, 7
    want = oracle.render(tris, mats, w, h, frames)
    with options(device, CHUNK_FRAMES=2, ACCEL=accel):
        got, st = render(device, tris, mats, w, h, frames, want_stats=True)
    assert_fb_equal(got, want, "soup(600), PT_OPT_ACCEL %d" % accel)
    assert int(st[shim.PT_STAT_SAMPLES]) == w * h * frames


@pytest.mark.parametrize("ring_bytes,form", [(1 << 32, "short"), ((1 << 32) + 512, "long")])
def test_offsets_above_2_31_and_the_long_form(cornell, cornell_33x97, ring_bytes, form):
    """A path carries a 32-bit BYTE offset from the ring's base while the whole ring is at most 4 GiB.  At exactly 4 GiB the upper slot
    begins at byte 2^31: every offset into it has its top bit set (a sign extension would store 4 GiB below the ring).  256 bytes more
    per slot and the render takes the long form, which carries the local pixel.  Seven frames in chunks of three: slots 0, 1, 0."""
    tris, mats = cornell
    dev = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    try:
        base = dev.getWorkspaceMemory()
        dev.reserveStaging(ring_bytes)
        assert dev.getWorkspaceMemory() - base == ring_bytes, "the ring is not the size the case is about"
        with options(dev, CHUNK_FRAMES=3):
            got = render(dev, tris, mats, W, H, 7)
    finally:
        adl.DeviceUtils.deallocate(dev)      # (releases the ring)
    assert_fb_equal(got, cornell_33x97[7], "%s form, a ring of %d bytes" % (form, ring_bytes))


def test_a_material_id_out_of_range_is_clamped(device, oracle):
    """The gather of a hit's material clamps a corrupt id to [0, materials - 1]: the image is the oracle's of the scene with the ids
    clamped beforehand (the oracle itself trusts them)."""
    tris, mats = scenes.variant("quads_scaled")
    bad = tris.copy()
    bad["id"][6] = len(mats) + 1000
    bad["id"][7] = 0x7fffffff
    bad["id"][20] = -3
    clamped = bad.copy()
    clamped["id"] = np.clip(bad["id"], 0, len(mats) - 1)
    assert (clamped["id"] != bad["id"]).sum() == 3
    w, h, frames = 48, 40, 4
    want = oracle.render(clamped, mats, w, h, frames)
    assert not np.array_equal(want, oracle.render(tris, mats, w, h, frames)), "the corrupt triangles are not in view"
    assert_fb_equal(render(device, bad, mats, w, h, frames), want, "material ids out of range")


def test_gathers_at_the_tiled_kernels_upper_end(device, oracle):
    """468 triangles (13 nested Cornell boxes): the largest brute-force scene of the suite, its last records 29 KB into the table."""
    tris, mats = scenes.nested_boxes(13)
    assert len(tris) == 468
    w, h, frames = 48, 40, 3
    assert_fb_equal(render(device, tris, mats, w, h, frames), oracle.render(tris, mats, w, h, frames), "nested_boxes(13)")
