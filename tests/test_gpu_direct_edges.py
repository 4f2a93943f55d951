"""Direct illumination (pt_render_direct) on the MI355X: the radiance BEFORE the fold, and the light sample's edges.

tests/test_gpu_direct.py compares framebuffers, pow(mean, 1 / 2.2) in binary32, and the fold hides errors: of the positive
radiance components of the Cornell box (64 x 64, frame 0, K = 4) about half keep their folded bits when they move by one ulp
(direct illumination).  The kernels write every sample's radiance L into the caller's workspace first (contract step 5 in
include/pt_shim.h), so here each render is compared twice, bit for bit, with tests/direct_oracle.c: the workspace with
``details()``'s L per (pixel, frame), and the framebuffer with ``render()``.

The inputs are those of tests/scenes.py's direct_* scenes; tests/test_direct_cpu.py proves without a GPU that each reaches the edge
it is named for (tl <= 0 beside searched rays, a light of no area, a list entry that is no emitter, a material of another type, a
camera outside the box, every roughness of the GGX guards, partial waves, K = 1 and 256)."""
import numpy as np
import pytest

import direct_oracle as do
from conftest import assert_fb_equal
from gpu_support import SEARCHES, lit_with_samples, options
from scenes import GLOSSY_SHIFTS, MIXED_SCALE, edge_scene

pytestmark = pytest.mark.gpu


def _want(name, W, H, frames, K, **stripes):
    tris, mats, lights, cam = edge_scene(name)[1]
    gid, frame = do.sample_ids(W, H, frames, **stripes)
    return (do.render(tris, mats, W, H, 0, frames, K, lights=lights, cam=cam, **stripes),
            do.details(tris, mats, W, H, gid, frame, K, lights=lights, cam=cam)[4].reshape(frames, -1, 3))


def wanted(key, W, H, frames, K, **stripes):
    """the restatement's (framebuffer, radiance [frames, local pixels, 3]) of a named input: computed once, shared, read-only"""
    return do.once(_want, key, W, H, frames, K, **stripes)


def check(device, key, scene4, W, H, frames, K, what, **stripes):
    """render; the workspace against the restatement's radiance, the framebuffer against its image"""
    want_fb, want_L = wanted(key, W, H, frames, K, **stripes)
    fb, ws = lit_with_samples(device, scene4, W, H, frames, K, **stripes)
    assert ws.shape == want_L.shape, what
    assert_fb_equal(ws, want_L, what + ": radiance before the fold")
    assert_fb_equal(fb, want_fb, what + ": framebuffer")


# ---- a. the radiance before the fold, on the inputs of tests/test_gpu_direct.py ---------------------------------------------------
@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_cornell_radiance_before_the_fold(device, quad, accel):
    key, sc = edge_scene("cornell")
    for W, H in ((64, 64), (40, 24)):
        for K in (1, 4):
            with options(device, QUAD_FILTER=quad, ACCEL=accel):
                check(device, key, sc, W, H, 4, K, "%dx%d K%d q%d a%d" % (W, H, K, quad, accel))


@pytest.mark.parametrize("copies,accel", [(10, 1), (15, 0), (15, 2), (15, 1)])
def test_nested_boxes_radiance_before_the_fold(device, copies, accel):
    """10 copies: the tiled brute-force table; 15: the LBVH (automatic and forced) and brute force over 540 triangles"""
    key, sc = edge_scene("nested:%d" % copies)
    with options(device, ACCEL=accel):
        check(device, key, sc, 32, 32, 2, 3, "nested_boxes(%d) accel %d" % (copies, accel))


# ---- b. stripes and chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
def test_stripes_hold_the_ranks_local_pixels(device, accel):
    """40 x 31 = 1 240 pixels: a partial last wave, checked against the restatement as a whole and rank by rank (rows of 5 over
    3 ranks: 11, 10 and 10 local rows -- 440, 400 and 400 local pixels, each with a partial wave of its own)"""
    key, sc = edge_scene("cornell")
    with options(device, ACCEL=accel):
        check(device, key, sc, 40, 31, 2, 2, "one rank, accel %d" % accel, stripe_rows=5)
        for rank in range(3):
            check(device, key, sc, 40, 31, 2, 2, "rank %d of 3, accel %d" % (rank, accel), stripe_rows=5, n_ranks=3, rank=rank)


def test_a_later_chunk_overwrites_slot_zero(device):
    """5 frames through a workspace of 2: launches of frames (0, 1), (2, 3), (4); slot 0 then holds frame 4 (slot 1 is not
    promised), and the framebuffer all five"""
    key, sc = edge_scene("cornell")
    W, H, K = 40, 31, 2
    want_fb, want_L = wanted(key, W, H, 5, K)
    fb, ws = lit_with_samples(device, sc, W, H, 5, K, chunk_frames=2)
    assert ws.shape == (2, W * H, 3)
    assert_fb_equal(ws[0], want_L[4], "slot 0 holds the last chunk's frame")
    assert_fb_equal(fb, want_fb, "five frames in chunks of two")


# ---- c. every scene of tests/scenes.py's direct_* family ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [MIXED_SCALE, -9])
def test_scaled_tiled_table(device, k):
    key, sc = edge_scene("scaled:10,%d" % k)
    with options(device, ACCEL=1):
        check(device, key, sc, 32, 32, 2, 3, "direct_scaled(10, %d), tiled brute force" % k)


@pytest.mark.parametrize("accel", [0, 2, 1])
@pytest.mark.parametrize("k", [MIXED_SCALE, -9])
def test_scaled_lbvh_and_brute_force(device, k, accel):
    """At the mixed scale a lane's shadow rays are searched, then not, then searched again: a fresh ray that searches nothing must
    end as a miss at the next refill -- were it to keep the hit of the ray before it (the primary hit, or an occluded shadow
    ray's), it would read as occluded and its light would be missing from the radiance.  At 2^-9 nothing is searched at all."""
    key, sc = edge_scene("scaled:15,%d" % k)
    with options(device, ACCEL=accel):
        check(device, key, sc, 32, 32, 2, 3, "direct_scaled(15, %d), accel %d" % (k, accel))


@pytest.mark.parametrize("quad,accel", SEARCHES)
@pytest.mark.parametrize("name", ["lights:list", "lights:36", "lights:10", "lights:all", "other_type", "from_behind", "scaled:1,-9"])
def test_edge_scenes(device, name, quad, accel):
    """the 36- and 37-triangle scenes, 64 x 64, K = 4, two frames, over every search"""
    key, sc = edge_scene(name)
    with options(device, QUAD_FILTER=quad, ACCEL=accel):
        check(device, key, sc, 64, 64, 2, 4, "%s q%d a%d" % (name, quad, accel))


# ---- d. K at its limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("K", [1, 256])
def test_light_samples_at_their_limits(device, K, accel):
    key, sc = edge_scene("cornell")
    with options(device, ACCEL=accel):
        check(device, key, sc, 16, 16, 1, K, "K %d accel %d" % (K, accel))


# ---- e. small and odd images -----------------------------------------------------------------------------------------------------------
SMALL = [(5, 3), (1, 1), (13, 5)]   # 15 samples: one partial wave; one sample; 65: a full wave and one lane


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_small_images_of_the_cornell_box(device, quad, accel):
    key, sc = edge_scene("cornell")
    for W, H in SMALL:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            check(device, key, sc, W, H, 2, 4, "%dx%d q%d a%d" % (W, H, quad, accel))


def test_small_images_through_the_lbvh(device):
    key, sc = edge_scene("nested:15")
    for W, H in SMALL:
        with options(device, ACCEL=2):
            check(device, key, sc, W, H, 2, 4, "nested_boxes(15) %dx%d" % (W, H))


# ---- f. the GGX branch at every roughness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("shift", GLOSSY_SHIFTS)
def test_glossy_rooms(device, shift, accel):
    """pt_direct_light's three quotients and max(E + S / K, 0) with the roughnesses on both sides of every guard, r = 0 included"""
    key, sc = edge_scene("glossy:%d" % shift)
    with np.errstate(all="ignore"):
        with options(device, ACCEL=accel):
            check(device, key, sc, 64, 48, 2, 4, "glossy_room(%d) accel %d" % (shift, accel))
