"""The CPU restatement of pt_render_indirect (tests/indirect_oracle.c) against the statements it repeats, without a GPU.

Two identities pin it bit for bit: with no lights it is the oracle's renderer at the same depth (ptor_render), at one bounce it is
direct illumination's restatement (odi_render).  One statistical check covers what neither identity reaches -- light samples at
later vertices, weighted by the path's mask, in place of the emission found by BRDF rays: the light-sampled estimator and the plain
one must have the same mean."""
import numpy as np
import pytest

import direct_oracle as do
import indirect_oracle as io
from conftest import assert_fb_equal
import indirect_edges as ie
from indirect_scenes import diffuse_cornell
from scenes import (FINITE_ROUGHNESS, FINITE_SHIFTS, GLOSSY_SHIFTS, MIXED_SCALE, ROUGHNESS, direct_light_list, edge_scene,
                    glossy_room)

W, H, FRAMES = 40, 24, 3
NONE = np.zeros(0, np.int32)


@pytest.mark.parametrize("B", [1, 2, 16])
@pytest.mark.parametrize("name", ["cornell", "glossy_room"])
def test_no_lights_is_the_renderer(oracle, cornell, name, B):
    tris, mats = cornell if name == "cornell" else glossy_room(0)
    want = oracle.render(tris, mats, W, H, FRAMES, max_bounces=B)
    for K in (1, 4):   # (K is not looked at without lights)
        assert_fb_equal(io.render(tris, mats, W, H, 0, FRAMES, K, B, lights=NONE), want, "%s B%d K%d" % (name, B, K))


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name", ["cornell", "light_list"])
def test_one_bounce_is_direct_illumination(cornell, name, K):
    if name == "cornell":
        tris, mats = cornell
        lights = None
    else:
        tris, mats, lights, _ = direct_light_list()
    want = do.render(tris, mats, W, H, 0, FRAMES, K, lights=lights)
    assert_fb_equal(io.render(tris, mats, W, H, 0, FRAMES, K, 1, lights=lights), want, "%s K%d" % (name, K))


def test_the_comparison_is_not_vacuous(oracle, cornell):
    """On the Cornell box at B = 16, K = 1 -- the GPU test's input -- the image is neither the renderer's nor direct illumination's,
    every reason for a path's end occurs, some path reaches vertex B, and light samples at later vertices are occluded and open."""
    tris, mats = cornell
    B, frames = 16, 5
    got = io.render(tris, mats, W, H, 0, frames, 1, B)
    assert not np.array_equal(got, oracle.render(tris, mats, W, H, frames, max_bounces=B))
    assert not np.array_equal(got, do.render(tris, mats, W, H, 0, frames, 1))
    gid, frame = io.all_samples(W, H, frames)
    rad, vertices, end, later = io.samples(tris, mats, W, H, gid, frame, 1, B)
    counts = {"miss": int((end == io.END_MISS).sum()), "pdf": int((end == io.END_PDF).sum()), "depth": int((end == io.END_DEPTH).sum()),
              "reached B": int((vertices == B).sum()), "later open": int(later[:, 0].sum()), "later occluded": int(later[:, 1].sum())}
    print(counts)
    assert all(v > 0 for v in counts.values()), counts
    assert vertices.max() == B and np.isfinite(rad).all()


# ---- unbiasedness ---------------------------------------------------------------------------------------------------------------
# The per-sample radiance before the fold of the all-diffuse Cornell box at B = 4, averaged over a 16 x 16 image and N frames.
# How N and the scale were obtained, with the oracle's PLAIN estimator (lights = []) alone: scale = |mean over frames [0, N) - mean
# over frames [N, 2N)| per channel; N = 200, 400, 800, ... doubled until every channel's scale is below 2 % of its mean.  200 .. 1600
# leave a channel at 2.2 %, 3.8 %, 2.3 %, 2.1 %; N = 3200 is the first to pass, with the figures below (1.4 %, 0.9 %, 1.2 % of the
# mean 1.296, 1.238, 1.016).  The test computes the scale again and checks the constants, so they cannot go stale.
# The light-sampled estimator is NOT the quieter of the two here: the box's light hangs 0.008 below the ceiling, and a light
# sample from a ceiling vertex above it has 1 / d^2 up to 1 / 6.4e-5.  Its value is bounded (about 4.7e5) and its mean right, but one
# such sample (3.76e5, pixel 23 of frame 6065) moves a mean over 256 x 6400 samples by 0.23: at N = 6400 the difference of the two
# estimators is 0.25 against a scale of 0.003.  Up to frame 3200 no such sample occurs.
UNBIASED_N = 3200
UNBIASED_SCALE = (0.01835795, 0.01169497, 0.01260588)


def _mean_radiance(tris, mats, lights, frame_begin, frames):
    gid, frame = io.all_samples(16, 16, frames, frame_begin)
    return io.samples(tris, mats, 16, 16, gid, frame, 1, 4, lights=lights)[0].astype(np.float64).mean(0)


def test_light_sampling_is_unbiased():
    tris, mats = diffuse_cornell()
    N = UNBIASED_N
    plain = _mean_radiance(tris, mats, NONE, 0, N)
    scale = np.abs(plain - _mean_radiance(tris, mats, NONE, N, N))
    nee = _mean_radiance(tris, mats, None, 0, N)
    print("N", N, "plain", plain, "scale", scale, "light-sampled", nee, "difference", np.abs(nee - plain))
    assert np.allclose(scale, UNBIASED_SCALE, rtol=1e-4, atol=0), "the recorded scale is stale: %s" % scale
    assert (scale < 0.02 * plain).all(), scale / plain
    assert (np.abs(nee - plain) <= 3.0 * scale).all(), (np.abs(nee - plain), 3.0 * scale)


# ---- each input of tests/test_gpu_indirect_edges.py reaches its edge ----------------------------------------------------------------
# The restatement alone, no GPU: a bit-exact comparison on an input that never reaches the edge it is rendered for proves nothing,
# so every floor below is a condition on the input (tests/indirect_edges.py: the scenes and sizes the device renders), found with
# io.details, not a measurement of the code under test.
U, O, C = do.OPEN_UNSEARCHED, do.R_OPEN, do.R_OCCLUDED


def _later_counts(reason):
    """{reason name: light samples at vertices i >= 1 that ended so}"""
    return do.count_reasons(reason[:, 1:, :])


def _bounced(mtype, end):
    """[n, V]: the path took a BRDF sample at vertex i and went on to the search of loop index i + 1"""
    return (mtype != 0) & (np.arange(mtype.shape[1])[None, :] < end[:, 1:2])


def test_details_is_the_walk_of_samples(cornell):
    """oii_details and oii_samples are outputs of one oii_sample: the same radiance, end and vertex count, and the reason codes fold
    back into the later-vertex counts"""
    tris, mats = cornell
    gid, frame = io.all_samples(W, H, 4)
    for K, B in ((1, 16), (4, 3)):
        rad, vertices, end, later = io.samples(tris, mats, W, H, gid, frame, K, B)
        mtype, flipped, emissive, reason, end2, rad2, nonfinite, material = io.details(tris, mats, W, H, gid, frame, K, B)
        V = min(B, io.DETAIL_VERTICES)
        assert reason.shape == (len(gid), V, K) and mtype.shape == (len(gid), V)
        assert np.array_equal(rad.view(np.uint32), rad2.view(np.uint32)) and np.array_equal(end, end2[:, 0])
        assert np.array_equal((mtype != 0).sum(axis=1), np.minimum(vertices, V))
        assert np.array_equal(mtype != 0, material >= 0) and np.array_equal(flipped, (mtype != 0).astype(np.uint8))
        assert np.array_equal(mtype[material >= 0], mats["type"][material[material >= 0]])
        assert np.array_equal(nonfinite != 0, ~np.isfinite(rad).all(axis=1))
        miss, pdf = end == io.END_MISS, end == io.END_PDF
        assert np.array_equal(end2[miss, 1], vertices[miss]) and np.array_equal(end2[pdf, 1], vertices[pdf] - 1)
        assert (end2[end == io.END_DEPTH, 1] == B - 1).all()
        assert ((reason != do.NOT_DRAWN).all(axis=2) == (mtype != 0)).all()     # K light samples at every vertex, none elsewhere
        if B <= V:
            assert np.array_equal(((reason[:, 1:] == O) | (reason[:, 1:] == U)).sum(axis=(1, 2)), later[:, 0])
            assert np.array_equal((reason[:, 1:] == C).sum(axis=(1, 2)), later[:, 1])


def _open_later_per_roughness(shift, K, B):
    """per FINITE_ROUGHNESS: the samples of the finite room ``shift`` with an OPEN light sample at a vertex i >= 1 on a surface of
    that roughness; the room's samples with a NaN or infinite component; its paths' largest count of bounces on GGX surfaces"""
    name, (tris, mats, _, _) = edge_scene("finite:%d" % shift)
    Wf, Hf, frames = ie.FINITE_SIZE
    mtype, _, _, reason, end, _, nonfinite, material = ie.details(name, Wf, Hf, frames, K, B)
    lit = (reason[:, 1:] == O).any(axis=2) & (mtype[:, 1:] == 2)
    rough = mats["roughness"][np.maximum(material[:, 1:], 0)]
    per = [int((lit & (rough == np.float32(r))).sum()) for r in FINITE_ROUGHNESS]
    return per, int(nonfinite.sum()), int((_bounced(mtype, end) & (mtype == 2)).sum(axis=1).max())


@pytest.mark.parametrize("K,B", ie.FINITE_KB)
def test_the_finite_rooms_are_finite_and_light_every_roughness(K, B):
    """40 x 24, 3 frames.  Measured for FINITE_SHIFTS = (5, 8), samples with an OPEN later light sample per finite roughness:
    K 1 / B 4: 31+0, 11+4, 26+232, 0+161, 0+19, 158+1, 267+0, 107+0, 0+84, 5+232, 65+12; K 2 / B 6: 34+0, 11+7, 39+254, 0+168,
    0+20, 146+3, 246+0, 96+0, 0+98, 5+232, 68+14; NaN or infinite samples 0; up to 4 (K 1 / B 4: B - 1 is 3) and 5 GGX bounces.
    No single shift of 0 .. 10 reaches all eleven, so a set of two is the smallest."""
    assert len(FINITE_ROUGHNESS) == 11 and len(set(np.float32(FINITE_ROUGHNESS).tolist())) == 11
    assert set(FINITE_ROUGHNESS) < set(ROUGHNESS) and min(FINITE_ROUGHNESS) > 2e-9 > max(set(ROUGHNESS) - set(FINITE_ROUGHNESS))
    per_shift = {shift: _open_later_per_roughness(shift, K, B) for shift in range(len(FINITE_ROUGHNESS))}
    for shift in FINITE_SHIFTS:
        per, nonfinite, ggx_bounces = per_shift[shift]
        print("finite room %d K%d B%d: OPEN at i >= 1 per roughness %s, non-finite samples %d, GGX bounces up to %d"
              % (shift, K, B, per, nonfinite, ggx_bounces))
        assert nonfinite == 0
        assert ggx_bounces >= 2
    total = np.sum([per_shift[shift][0] for shift in FINITE_SHIFTS], axis=0)
    assert (total >= 1).all(), total
    assert len(FINITE_SHIFTS) == 2 and not any(min(per) >= 1 for per, _, _ in per_shift.values()), "one shift would do"
    assert all(nonfinite == 0 for _, nonfinite, _ in per_shift.values())     # (the eleven are finite wherever they lie)


GLOSSY_NAN_SAMPLES = {0: 856, 1: 1787, 4: 348, 13: 1782}   # of 2 880, tests/test_gpu_indirect.py's test_glossy_room


def test_the_mixed_glossy_rooms_are_largely_nan():
    """On record, so that it cannot grow silently: in the rooms of all 17 roughnesses that test_glossy_room renders (40 x 24,
    3 frames, K = 1, B = 4) 30 %, 62 %, 12 % and 62 % of the samples hold a NaN -- the six roughnesses below 2e-9 make one of every
    path that bounces on them -- and a bit-exact comparison sees nothing of such a path after its first NaN.  The finite rooms
    above are what compares the other eleven roughnesses' quotients."""
    assert tuple(GLOSSY_NAN_SAMPLES) == GLOSSY_SHIFTS
    for shift, count in GLOSSY_NAN_SAMPLES.items():
        tris, mats = glossy_room(shift)
        gid, frame = io.all_samples(W, H, 3)
        rad = io.details(tris, mats, W, H, gid, frame, 1, 4)[5]
        nan = int(np.isnan(rad).any(axis=1).sum())
        print("glossy_room(%d): %d of %d samples hold a NaN (%.1f %%)" % (shift, nan, len(rad), 100.0 * nan / len(rad)))
        assert nan == count and len(rad) == 2880


def test_the_direct_glossy_rooms_hold_no_nan():
    """tests/test_gpu_direct_edges.py's glossy rooms (64 x 48, 2 frames, K = 4) for comparison: one vertex, no BRDF sample, and no
    sample with a NaN or infinite component in any of the four rooms (DESIGN.md records the share)"""
    for shift in GLOSSY_SHIFTS:
        tris, mats = glossy_room(shift)
        gid, frame = io.all_samples(64, 48, 2)
        L = do.details(tris, mats, 64, 48, gid, frame, 4)[4]
        bad = int((~np.isfinite(L)).any(axis=1).sum())
        print("direct illumination, glossy_room(%d): %d of %d samples not finite" % (shift, bad, len(L)))
        assert bad == 0


@pytest.mark.parametrize("copies", [15, 10])
def test_the_mixed_scale_leaves_later_shadow_rays_unsearched(copies):
    """direct_scaled(copies, MIXED_SCALE), 32 x 32, 2 frames, K 2, B 4 (two frames suffice for all four situations).  Measured at
    i >= 1, OPEN_UNSEARCHED / OPEN / OCCLUDED: 15 copies 2235 / 951 / 1316, 10 copies 1390 / 1718 / 1193.  Vertices i >= 1 whose
    unsearched sample directly follows a searched one: 246 and 168; a searched one directly after an unsearched one: 224 and 156;
    whose last cast light sample is unsearched and the next closest search hits: 752 and 473, misses: 163 and 113."""
    Ws, Hs, frames, K, B = ie.SCALED_SIZE
    assert K == 2
    mtype, _, _, reason, end, _, nonfinite, _ = ie.details("scaled:%d,%d" % (copies, MIXED_SCALE), Ws, Hs, frames, K, B)
    counts = _later_counts(reason)
    searched, unsearched = (reason == O) | (reason == C), reason == U
    after_searched = int((searched[:, 1:, 0] & unsearched[:, 1:, 1]).sum())
    before_searched = int((unsearched[:, 1:, 0] & searched[:, 1:, 1]).sum())
    last_unsearched = np.where(searched[:, :, 1] | unsearched[:, :, 1], unsearched[:, :, 1], unsearched[:, :, 0])   # the last CAST one
    then_hit = then_miss = 0
    for i in range(1, B - 1):
        then_hit += int((last_unsearched[:, i] & (mtype[:, i + 1] != 0)).sum())
        then_miss += int((last_unsearched[:, i] & (end[:, 0] == io.END_MISS) & (end[:, 1] == i + 1)).sum())
    print(copies, counts, after_searched, before_searched, then_hit, then_miss)
    assert min(counts["OPEN_UNSEARCHED"], counts["OPEN"], counts["OCCLUDED"]) >= 100, counts
    assert min(after_searched, before_searched, then_hit, then_miss) >= 10
    assert nonfinite.sum() == 0


@pytest.mark.parametrize("copies", [15, 10, 1])
def test_the_smallest_scale_searches_no_later_shadow_ray(copies):
    """k = -9: every cast light sample at i >= 1 is OPEN_UNSEARCHED (measured 1226, 1221 and 1348), none is occluded; the closest
    searches between them hit and miss (148 / 448 after an unsearched last sample at 15 copies)"""
    Ws, Hs, frames, K, B = ie.SCALED_SIZE
    mtype, _, _, reason, end, _, _, _ = ie.details("scaled:%d,-9" % copies, Ws, Hs, frames, K, B)
    counts = _later_counts(reason)
    print(copies, counts)
    assert counts["OPEN"] == 0 and counts["OCCLUDED"] == 0 and counts["OPEN_UNSEARCHED"] >= 1000, counts
    assert (mtype[:, 2] != 0).sum() >= 100 and ((end[:, 0] == io.END_MISS) & (end[:, 1] >= 2)).sum() >= 100


def test_the_light_lists_reach_their_edges_at_later_vertices():
    """40 x 24, 2 frames, K 4, B 4.  [36, 10, 10, 36, 3, 11]: 3 252 light samples at i >= 1 end as NAN.  Which entry a light sample
    draws shows in no output, but the draws do not depend on the list's content: with the wall's entry (3) replaced by the light of
    no area, exactly the samples that drew it turn NAN.  Measured: 1 585 of them at i >= 1, 1 157 of those cast a shadow ray.
    [36] alone: all 9 720 later light samples are NAN, yet the image is not the no-lights image: the uniforms are drawn and the
    emission of later vertices is withheld (877 framebuffer values differ).  Measured at i >= 1, [10]: NOT_FACING 1439, OPEN 7328,
    OCCLUDED 953; arange(37): NOT_FACING 1985, NAN 268, OPEN 3395, OCCLUDED 4072."""
    from scenes import LIGHT_LIST

    Wn, Hn, frames, K, B = ie.NAMED_SIZE
    name, (tris, mats, lights, _) = edge_scene("lights:list")
    reason = ie.details(name, Wn, Hn, frames, K, B)[3]
    counts = _later_counts(reason)
    assert counts["NAN"] >= 1000 and counts["OPEN"] >= 1000 and counts["OCCLUDED"] >= 100, counts
    assert tuple(lights) == LIGHT_LIST and LIGHT_LIST[4] == 3
    no_wall = np.array(LIGHT_LIST, np.int32)
    no_wall[4] = 36
    gid, frame = do.sample_ids(Wn, Hn, frames)
    reason2 = io.details(tris, mats, Wn, Hn, gid, frame, K, B, lights=no_wall)[3]
    assert np.array_equal(reason == do.NOT_DRAWN, reason2 == do.NOT_DRAWN), "the paths do not depend on the list"
    wall = (reason2 == do.NAN) & (reason != do.NAN)
    assert np.array_equal(reason[~wall], reason2[~wall])
    cast = wall & ((reason == O) | (reason == C))
    print("the wall's entry is drawn %d times at i >= 1, %d of them cast a shadow ray" % (int(wall[:, 1:].sum()), int(cast[:, 1:].sum())))
    assert int(cast[:, 1:].sum()) >= 500

    name, (tris, mats, lights, _) = edge_scene("lights:36")
    reason = ie.details(name, Wn, Hn, frames, K, B)[3]
    counts = _later_counts(reason)
    assert counts["NAN"] >= 5000 and set(np.unique(reason[:, 1:])) == {do.NOT_DRAWN, do.NAN}, counts
    fb = ie.wanted(name, Wn, Hn, frames, K, B)[0]
    none = io.render(tris, mats, Wn, Hn, 0, frames, K, B, lights=NONE)
    differ = int((fb.view(np.uint32) != none.view(np.uint32)).sum())
    print("[36] against no lights: %d framebuffer values differ" % differ)
    assert differ >= 100

    one = _later_counts(ie.details("lights:10", Wn, Hn, frames, K, B)[3])
    every = _later_counts(ie.details("lights:all", Wn, Hn, frames, K, B)[3])
    print(one, every)
    assert one["OPEN"] >= 1000 and one["OCCLUDED"] >= 100 and one["NAN"] == 0, one
    assert every["OPEN"] >= 1000 and every["OCCLUDED"] >= 1000 and every["NAN"] >= 100, every


def test_a_later_vertex_of_another_type_ends_the_path():
    """direct_other_type, 40 x 24, 2 frames, K 4, B 4: 83 vertices at i >= 1 lie on a type-3 material (the walls; the paths come
    from the glossy surfaces).  All K light samples there are OTHER_TYPE -- 3K uniforms drawn, nothing cast -- and the BRDF sample
    then ends the path at pdf <= 0 at that very vertex.  1 249 paths end with END_PDF (1 on the Cornell box at this size)."""
    Wn, Hn, frames, K, B = ie.NAMED_SIZE
    mtype, _, _, reason, end, _, _, _ = ie.details("other_type", Wn, Hn, frames, K, B)
    later3 = mtype[:, 1:] == 3
    assert int(later3.sum()) >= 50
    assert (reason[:, 1:][later3] == do.OTHER_TYPE).all()
    for i in range(1, B - 1):   # (at i == B - 1 the path ends by depth: no BRDF sample is taken)
        on3 = mtype[:, i] == 3
        assert ((end[on3, 0] == io.END_PDF) & (end[on3, 1] == i)).all()
    at_pdf = int((end[:, 0] == io.END_PDF).sum())
    plain = int((ie.details("cornell", Wn, Hn, frames, K, B)[4][:, 0] == io.END_PDF).sum())
    print("type 3 at i >= 1: %d vertices; END_PDF %d paths, %d on the Cornell box" % (int(later3.sum()), at_pdf, plain))
    assert at_pdf >= 1000 > 10 >= plain
    assert _later_counts(reason)["OPEN"] >= 50      # (the glossy surfaces keep their light)


def test_the_camera_outside_the_box_bounces_inside():
    """direct_from_behind: 810 of 1 920 samples miss, the others bounce on: 2 693 later vertices (every normal negated, as at every
    hit), OPEN 7768 and OCCLUDED 1503 light samples at them"""
    Wn, Hn, frames, K, B = ie.NAMED_SIZE
    mtype, flipped, _, reason, _, _, _, _ = ie.details("from_behind", Wn, Hn, frames, K, B)
    counts = _later_counts(reason)
    print(counts, int((mtype[:, 0] == 0).sum()), int((mtype[:, 1:] != 0).sum()))
    assert 100 < int((mtype[:, 0] == 0).sum()) < len(mtype) - 500
    assert np.array_equal(flipped != 0, mtype != 0) and int((mtype[:, 1:] != 0).sum()) >= 1000
    assert counts["OPEN"] >= 1000 and counts["OCCLUDED"] >= 100, counts


def test_a_path_runs_into_the_light_at_a_later_vertex(cornell):
    """The Cornell box at tests/test_gpu_indirect.py's size (40 x 24, 4 frames): vertices at i >= 1 that lie on the emitter while
    the light list is not empty, where :241 must NOT be added.  Measured among the first 8 vertices: 63 at (B 16, K 1), 30 at
    (B 3, K 4)."""
    tris, mats = cornell
    gid, frame = io.all_samples(W, H, 4)
    for B, K in ((16, 1), (3, 4)):
        emissive = io.details(tris, mats, W, H, gid, frame, K, B)[2]
        print("B %d K %d: %d later vertices on the emitter" % (B, K, int(emissive[:, 1:].sum())))
        assert int(emissive[:, 1:].sum()) >= 10


@pytest.mark.parametrize("name", ie.SMALL_SCENES)
def test_the_small_images_hold_paths_of_every_length(name):
    """5 x 3 (one partial wave) and 13 x 5 (a full wave and one lane), 2 frames, K 4, B 4: paths of 0, 1, 2, 3 and 4 vertices in one
    wave, ended by a miss and by the depth.  Measured, samples per vertex count: Cornell box 8 / 3 / 2 / 4 / 13 and 73 / 20 / 11 /
    5 / 21, nested_boxes(15) 8 / 9 / 6 / 1 / 6 and 73 / 25 / 6 / 7 / 19."""
    for Ws, Hs, B in ie.SMALL:
        mtype, _, _, _, end, _, _, _ = ie.details(name, Ws, Hs, 2, 4, B)
        per = np.bincount((mtype != 0).sum(axis=1), minlength=5)
        print(name, Ws, Hs, B, per, np.bincount(end[:, 0], minlength=3))
        if (Ws, Hs) != (1, 1):
            assert B == 4 and (Ws * Hs) % 64 != 0 and (per > 0).all(), per
            assert (end[:, 0] == io.END_MISS).any() and (end[:, 0] == io.END_DEPTH).any()


def test_the_striped_image_has_partial_waves():
    """40 x 31 in rows of 5 over 3 ranks: 11, 10 and 10 local rows; the whole image and every rank end in a partial wave"""
    Ws, Hs, _, _, _ = ie.STRIPED_SIZE
    local = [len(do.local_gids(Ws, Hs, stripe_rows=ie.STRIPE_ROWS, n_ranks=ie.RANKS, rank=r)) for r in range(ie.RANKS)]
    assert (Ws * Hs) % 64 == 24 and local == [440, 400, 400] and [n % 64 for n in local] == [56, 16, 16]


def test_the_limits_of_k_and_b(cornell):
    """16 x 16, one frame.  B = 65535 is B = 64 in the restatement, bit for bit: the longest path has 45 vertices.  K = 256 at
    B = 3: 67 611 open and 8 295 occluded light samples at i >= 1 (K = 1: 266 and 33)."""
    tris, mats = cornell
    Wl, Hl, frames = ie.LIMITS_SIZE
    assert ie.LIMITS_KB == ((1, 3), (256, 3), (1, 65535), (1, 64))
    for a, b in zip(ie.wanted("cornell", Wl, Hl, frames, 1, 65535), ie.wanted("cornell", Wl, Hl, frames, 1, 64)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    gid, frame = do.sample_ids(Wl, Hl, frames)
    longest = int(io.samples(tris, mats, Wl, Hl, gid, frame, 1, 65535)[1].max())
    print("the longest path has %d vertices" % longest)
    assert 16 < longest < 64
    for K in (1, 256):
        later = io.samples(tris, mats, Wl, Hl, gid, frame, K, 3)[3].sum(axis=0)
        print("K %d B 3: later open %d, occluded %d" % (K, later[0], later[1]))
        assert later[0] >= 100 and later[1] >= 10


def test_the_clamped_list_differs_from_the_emitters(cornell):
    """[-1, 10, ntri + 5, 11] clamps to [0, 10, 35, 11]: half the draws go to two walls, and the image is not the emitters' own"""
    tris, mats = cornell
    Wc, Hc, frames, K, B = ie.CLAMPED_SIZE
    name, (_, _, clamped, _) = ie.clamped_scene()
    assert clamped.tolist() == [0, 10, len(tris) - 1, 11] and ie.clamped_raw(len(tris)) != clamped.tolist()
    counts = _later_counts(ie.details(name, Wc, Hc, frames, K, B)[3])
    assert counts["OPEN"] >= 100 and counts["OCCLUDED"] >= 100, counts
    assert not np.array_equal(ie.wanted(name, Wc, Hc, frames, K, B)[0], io.render(tris, mats, Wc, Hc, 0, frames, K, B))
