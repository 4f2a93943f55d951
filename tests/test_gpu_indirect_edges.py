"""Indirect illumination (pt_render_indirect) on the MI355X at the edges tests/test_gpu_indirect.py does not reach: light samples at
LATER vertices that search nothing, that meet a light of no area, a list entry that is no emitter or a material of another type;
glossy rooms whose paths stay finite; images with partial waves; stripes and chunks; K and B at their limits; clamped light indices.

Every check compares the sample workspace with the restatement's radiance before the fold and the framebuffer with its image, bit for
bit (tests/indirect_oracle.c), in the shape of tests/test_gpu_direct_edges.py's ``check``.  The inputs are tests/indirect_edges.py's;
tests/test_indirect_cpu.py proves without a GPU, on exactly these scenes and sizes, that each reaches the edge it is rendered for."""
import numpy as np
import pytest

import indirect_edges as ie
from conftest import assert_fb_equal
from gpu_support import SEARCHES, LitBuffers, lit_with_samples, options
from oclpathtracer_amd import shim
from scenes import FINITE_SHIFTS, MIXED_SCALE

pytestmark = pytest.mark.gpu


def check(device, name, W, H, frames, K, B, what, **stripes):
    """render; the workspace against the restatement's radiance, the framebuffer against its image"""
    want_fb, want_L = ie.wanted(name, W, H, frames, K, B, **stripes)
    fb, ws = lit_with_samples(device, ie.scene_of(name)[1], W, H, frames, K, max_bounces=B, **stripes)
    assert ws.shape == want_L.shape, what
    assert_fb_equal(ws, want_L, what + ": radiance before the fold")
    assert_fb_equal(fb, want_fb, what + ": framebuffer")


# ---- finite glossy rooms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("K,B", ie.FINITE_KB)
@pytest.mark.parametrize("shift", FINITE_SHIFTS)
def test_finite_glossy_rooms(device, shift, K, B, accel):
    """pt_indirect_bounce's guarded quotients at every roughness that keeps a path finite, feeding light samples at later vertices:
    no sample is NaN or infinite, so every bit of every path is compared"""
    W, H, frames = ie.FINITE_SIZE
    with options(device, ACCEL=accel):
        check(device, "finite:%d" % shift, W, H, frames, K, B, "finite room %d K%d B%d accel %d" % (shift, K, B, accel))


# ---- scaled scenes: shadow rays that search nothing, at later vertices ---------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 2, 1])
@pytest.mark.parametrize("k", [MIXED_SCALE, -9])
def test_scaled_lbvh_and_brute_force(device, k, accel):
    """PtIndirectWork::next_ray after a shadow ray with tl <= 0: it was not searched and must read as open -- not as the hit of the
    search before it, the vertex's own closest hit or an occluded shadow ray's -- and the next light sample, or the BRDF sample and
    its closest search, follow.  At 2^-9 no shadow ray is searched at all."""
    W, H, frames, K, B = ie.SCALED_SIZE
    with options(device, ACCEL=accel):
        check(device, "scaled:15,%d" % k, W, H, frames, K, B, "direct_scaled(15, %d), accel %d" % (k, accel))


@pytest.mark.parametrize("k", [MIXED_SCALE, -9])
def test_scaled_tiled_table(device, k):
    W, H, frames, K, B = ie.SCALED_SIZE
    with options(device, ACCEL=1):
        check(device, "scaled:10,%d" % k, W, H, frames, K, B, "direct_scaled(10, %d), tiled brute force" % k)


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_scaled_cornell_box(device, quad, accel):
    W, H, frames, K, B = ie.SCALED_SIZE
    with options(device, QUAD_FILTER=quad, ACCEL=accel):
        check(device, "scaled:1,-9", W, H, frames, K, B, "direct_scaled(1, -9) q%d a%d" % (quad, accel))


# ---- the named edge scenes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,accel", SEARCHES)
@pytest.mark.parametrize("name", ie.NAMED)
def test_edge_scenes(device, name, quad, accel):
    """light lists with a light of no area and a wall in them, a material of another type (the path ends at pdf <= 0 after the
    vertex's 3K uniforms and the bounce's two), the camera behind the box -- through the bounce loop, over every search"""
    W, H, frames, K, B = ie.NAMED_SIZE
    with options(device, QUAD_FILTER=quad, ACCEL=accel):
        check(device, name, W, H, frames, K, B, "%s q%d a%d" % (name, quad, accel))


# ---- small and odd images: partial waves through the lock-step bounce loop ---------------------------------------------------------------
@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_small_images_of_the_cornell_box(device, quad, accel):
    for W, H, B in ie.SMALL:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            check(device, "cornell", W, H, 2, 4, B, "%dx%d B%d q%d a%d" % (W, H, B, quad, accel))


def test_small_images_through_the_lbvh(device):
    for W, H, B in ie.SMALL:
        with options(device, ACCEL=2):
            check(device, "nested:15", W, H, 2, 4, B, "nested_boxes(15) %dx%d B%d" % (W, H, B))


# ---- stripes and chunks, against the restatement and before the fold ------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
def test_stripes_hold_the_ranks_local_pixels(device, accel):
    """40 x 31: a partial last wave, as one rank and rank by rank (440, 400 and 400 local pixels, each with a partial wave)"""
    W, H, frames, K, B = ie.STRIPED_SIZE
    with options(device, ACCEL=accel):
        check(device, "cornell", W, H, frames, K, B, "one rank, accel %d" % accel, stripe_rows=ie.STRIPE_ROWS)
        for rank in range(ie.RANKS):
            check(device, "cornell", W, H, frames, K, B, "rank %d of %d, accel %d" % (rank, ie.RANKS, accel),
                  stripe_rows=ie.STRIPE_ROWS, n_ranks=ie.RANKS, rank=rank)


def test_a_later_chunk_overwrites_slot_zero(device):
    """5 frames through a workspace of 2: launches of frames (0, 1), (2, 3), (4); slot 0 then holds frame 4 (slot 1 is not
    promised), and the framebuffer all five"""
    W, H, _, K, B = ie.STRIPED_SIZE
    want_fb, want_L = ie.wanted("cornell", W, H, ie.CHUNKED_FRAMES, K, B)
    fb, ws = lit_with_samples(device, ie.scene_of("cornell")[1], W, H, ie.CHUNKED_FRAMES, K, chunk_frames=2, max_bounces=B)
    assert ws.shape == (2, W * H, 3)
    assert_fb_equal(ws[0], want_L[4], "slot 0 holds the last chunk's frame")
    assert_fb_equal(fb, want_fb, "five frames in chunks of two")


def test_a_render_continued_at_frame_two(device):
    """frames (0, 1), then a call that begins at frame 2: its three frames fill the workspace from slot 0, the framebuffer holds
    all five"""
    from oclpathtracer_amd.indirect import IndirectRenderer

    W, H, _, K, B = ie.STRIPED_SIZE
    want_fb, want_L = ie.wanted("cornell", W, H, ie.CHUNKED_FRAMES, K, B)
    tris, mats, _, _ = ie.scene_of("cornell")[1]
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, stripe_rows=1, chunk_frames=3)
    try:
        r.render(2, 0)
        r.render(3, 2)
        fb = r.read()
        ws = np.zeros((3, W * H, 3), np.float32)
        r.samples.read(ws, ws.size)
        device.waitForCompletion()
    finally:
        r.release()
    assert_fb_equal(ws, want_L[2:5], "frames 2, 3 and 4 before the fold")
    assert_fb_equal(fb, want_fb, "two frames, then three from frame_begin = 2")


# ---- K and B at their limits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("K,B", ie.LIMITS_KB)
def test_light_samples_and_bounces_at_their_limits(device, K, B, accel):
    """K = 1 and 256 at B = 3; B = 65535, where every path ends long before (the longest has 45 vertices), and B = 64"""
    W, H, frames = ie.LIMITS_SIZE
    with options(device, ACCEL=accel):
        check(device, "cornell", W, H, frames, K, B, "K %d B %d accel %d" % (K, B, accel))


# ---- light indices out of range, through the raw C ABI --------------------------------------------------------------------------------
def test_light_indices_are_clamped_where_they_are_used(device):
    W, H, frames, K, B = ie.CLAMPED_SIZE
    name, (tris, mats, clamped, _) = ie.clamped_scene()
    raw = ie.clamped_raw(len(tris))
    assert clamped.tolist() == [0, 10, len(tris) - 1, 11]
    want_fb, want_L = ie.wanted(name, W, H, frames, K, B)
    b = LitBuffers("pt_render_indirect", device, tris, mats, W, H, lights=raw, frames=frames, pad=0)
    try:
        assert b.call(b.params(len(raw), light_samples=K, max_bounces=B, frame_count=frames)) == shim.PT_OK
        fb = b.read()
        ws = b.read(b.sb, np.zeros((frames, W * H, 3), np.float32))
    finally:
        b.release()
    assert_fb_equal(ws, want_L, "clamped lights: radiance before the fold")
    assert_fb_equal(fb, want_fb, "clamped lights: framebuffer")
