"""The CPU restatement of pt_render_indirect_mis (tests/mis_oracle.c) against the statements it repeats and against the plain
light-sampling estimator (tests/indirect_oracle.c), without a GPU.

Identities pin it bit for bit where the weights play no part.  What they do not reach -- the weights themselves -- is statistical:
the MIS estimator has the plain one's mean on glossy rooms of three roughnesses, keeps that mean under wrong light lists that move
the plain estimator's by many standard errors (the check that fails when the counts are ignored), and has a fraction of its
variance where glossy surfaces lie beside the light.  The last part proves that each input of tests/test_gpu_mis.py reaches the
edge it is rendered for."""
import numpy as np
import pytest

import direct_oracle as do
import indirect_oracle as io
import mis_cases as mc
import mis_oracle as mo
from conftest import assert_fb_equal
from scenes import direct_light_list, edge_scene, glossy_room

W, H, FRAMES = mc.W, mc.H, mc.FRAMES
NONE = np.zeros(0, np.int32)


# ---- identities, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 16])
@pytest.mark.parametrize("name", ["cornell", "glossy_room"])
def test_no_lights_is_the_renderer(oracle, cornell, name, B):
    tris, mats = cornell if name == "cornell" else glossy_room(0)
    want = oracle.render(tris, mats, W, H, FRAMES, max_bounces=B)
    for K in (1, 4):   # (K is not looked at without lights; neither are the counts)
        assert_fb_equal(mo.render(tris, mats, W, H, 0, FRAMES, K, B, lights=NONE), want, "%s B%d K%d" % (name, B, K))


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name", ["cornell", "light_list"])
def test_one_bounce_is_direct_illumination(cornell, name, K):
    if name == "cornell":
        tris, mats = cornell
        lights = None
    else:
        tris, mats, lights, _ = direct_light_list()
    want = do.render(tris, mats, W, H, 0, FRAMES, K, lights=lights)
    assert_fb_equal(mo.render(tris, mats, W, H, 0, FRAMES, K, 1, lights=lights), want, "%s K%d" % (name, K))


@pytest.mark.parametrize("K,B", [(1, 16), (4, 4), (2, 2)])
def test_a_sample_without_weights_is_the_plain_one(cornell, K, B):
    """A sample none of whose light samples is WEIGHTED and that has no later emissive hit is indirect_oracle's, bit for bit; the
    others are what the comparison with the device is about, so there must be many, and many of them must differ in bits."""
    tris, mats = cornell
    gid, frame = io.all_samples(W, H, FRAMES)
    rad, vertices, end, later, mis = mo.samples(tris, mats, W, H, gid, frame, K, B)
    prad, pvertices, pend, plater = io.samples(tris, mats, W, H, gid, frame, K, B)
    assert np.array_equal(vertices, pvertices) and np.array_equal(end, pend) and np.array_equal(later, plater)   # the same walk
    same = (mis[:, 0] == 0) & (mis[:, 1] == 0)
    differ = (rad.view(np.uint32) != prad.view(np.uint32)).any(axis=1)
    print("K %d B %d: %d of %d samples carry no weight; %d of the others differ in bits" % (K, B, same.sum(), len(same), differ[~same].sum()))
    assert np.array_equal(rad[same].view(np.uint32), prad[same].view(np.uint32))
    assert same.sum() >= 100 and differ[~same].sum() >= 100
    # details is the same walk as samples
    d = mo.details(tris, mats, W, H, gid, frame, K, B)
    assert np.array_equal(d[5].view(np.uint32), rad.view(np.uint32))
    if B <= mo.DETAIL_VERTICES:
        assert np.array_equal((d[8] == mo.WEIGHTED).sum(axis=(1, 2)), mis[:, 0]) and np.array_equal((d[9] >= 0).sum(axis=1), mis[:, 1])


# ---- the statistics ------------------------------------------------------------------------------------------------------------
# 16 x 16, K = 1, B = 4, N = 3200 frames per estimate: the size of test_indirect_cpu's unbiasedness check.  A standard error is taken
# from the variance of the N per-frame image means (frames are independent; pixels of one frame need not be).
N, SW, SH, SK, SB = 3200, 16, 16, 1, 4
E0, E1 = 10, 11   # the Cornell box's emitters


def _room(r):
    return glossy_room(0, [r])


_RAD = {}


def _radiance(scene, frame_begin, mis, lights=None):
    """float64 [N, pixels, 3] of frames [frame_begin, frame_begin + N), computed once per (scene, range, estimator, list)"""
    k = (scene, frame_begin, mis, lights)
    if k not in _RAD:
        tris, mats = edge_scene("cornell")[1][:2] if scene == "cornell" else _room(scene)
        _RAD[k] = mo.radiance_frames(tris, mats, SW, SH, frame_begin, N, SK, SB, mis=mis, lights=None if lights is None else np.asarray(lights, np.int32))
        _RAD[k].setflags(write=False)
    return _RAD[k]


def _mean_se(rad):
    per_frame = rad.mean(axis=1)
    return per_frame.mean(axis=0), per_frame.std(axis=0, ddof=1) / np.sqrt(len(per_frame))


def _z(a, b):
    (ma, sa), (mb, sb) = _mean_se(a), _mean_se(b)
    return np.abs(ma - mb) / np.sqrt(sa ** 2 + sb ** 2)


@pytest.mark.parametrize("r", [0.3, 0.05, 0.008])
def test_mis_is_unbiased_against_light_sampling(r):
    """MIS on frames [N, 2N) against the plain restatement on frames [0, N): per channel the image means differ by at most 3
    combined standard errors (a z-bound over nine comparisons).  Measured: 0.31 0.47 0.64 (r 0.3), 0.77 0.82 0.86 (0.05), 0.24 0.35
    0.30 (0.008)."""
    z = _z(_radiance(r, N, True), _radiance(r, 0, False))
    print("roughness %g: |difference of means| in standard errors per channel %s" % (r, z))
    assert (z <= 3.0).all(), z


def test_mis_is_robust_to_a_wrong_light_list():
    """The r = 0.008 room with a duplicated entry, a missing emitter, and the list reversed and doubled, each on frames of its own:
    the MIS means stay within 3 standard errors of the correct list's MIS mean (frames [N, 2N)), the plain estimator's are more than
    3 off in some channel.  With the counts ignored (all 1) MIS would share the plain estimator's error on the first and third list.
    Measured, worst channel, MIS / plain: 0.32 / 4.19, 1.15 / 7.39, 0.49 / 7.04."""
    right = _radiance(0.008, N, True)
    for k, lights in enumerate([(E0, E1, E0), (E0,), (E1, E0, E0, E1)]):
        begin = (2 + k) * N
        zm, zp = _z(_radiance(0.008, begin, True, lights), right), _z(_radiance(0.008, begin, False, lights), right)
        print("list %s: MIS %s, plain %s standard errors from the correct list's mean" % (list(lights), zm, zp))
        assert (zm <= 3.0).all(), (lights, zm)
        assert (zp > 3.0).any(), (lights, zp)


def _variance(rad):
    return float(rad.var(axis=0).mean())   # per pixel and channel over the frames, then the mean


@pytest.mark.parametrize("scene,floor", [("cornell", 2.0), (0.008, 4.0)])
def test_mis_lowers_the_variance_beside_the_light(scene, floor):
    """Mean per-pixel variance of the per-sample radiance over frames [0, N), plain / MIS on the same frames.  Measured: Cornell box
    109.2 / 40.2 = 2.72, r = 0.008 room 234.5 / 41.9 = 5.59 (DESIGN.md S4 carries them)."""
    plain, mis = _variance(_radiance(scene, 0, False)), _variance(_radiance(scene, 0, True))
    print("%s: variance plain %.4g, MIS %.4g, ratio %.3f" % (scene, plain, mis, plain / mis))
    assert plain / mis >= floor


@pytest.mark.parametrize("scene", [0.05, 0.3, "diffuse"])
def test_mis_changes_nothing_where_brdf_rays_do_not_find_the_light(scene):
    """On record, not a bound on the estimator: at roughness 0.05 and 0.3 and on the all-diffuse box the two variances agree to
    1 % (measured ratios 1.001, 1.000, 1.000) -- MIS costs nothing there, and gains nothing."""
    if scene == "diffuse":
        from indirect_scenes import diffuse_cornell

        tris, mats = diffuse_cornell()
        plain = _variance(mo.radiance_frames(tris, mats, SW, SH, 0, N, SK, SB, mis=False))
        mis = _variance(mo.radiance_frames(tris, mats, SW, SH, 0, N, SK, SB))
    else:
        plain, mis = _variance(_radiance(scene, 0, False)), _variance(_radiance(scene, 0, True))
    print("%s: variance plain %.5g, MIS %.5g, ratio %.4f" % (scene, plain, mis, plain / mis))
    assert 0.99 <= plain / mis <= 1.01


# ---- each input of tests/test_gpu_mis.py reaches its edge ----------------------------------------------------------------------------
def test_every_gpu_input_is_finite():
    """The count of samples with a NaN or infinite component, per input of the GPU module: 0 on every one of them (the Cornell box,
    finite:5, finite:8, nested:10, nested:15 and the five lists), so a bit-exact comparison sees every path whole."""
    for scene, lights, Ws, Hs, frames, K, B, stripes in mc.cases():
        nonfinite = mc.details(scene, lights, Ws, Hs, frames, K, B, **stripes)[6]
        assert int(nonfinite.sum()) == 0, (scene, lights, Ws, Hs, frames, K, B, int(nonfinite.sum()))


def _edges(scene, lights, K, B):
    mtype, _, _, reason, _, _, _, _, weight, count, wb = mc.details(scene, lights, W, H, FRAMES, K, B)
    cast = (reason == do.R_OPEN) | (reason == do.OPEN_UNSEARCHED) | (reason == do.R_OCCLUDED)
    assert np.array_equal(weight != mo.W_NONE, cast)              # a weight code exactly where a light sample reached its weight
    out = {name: int((weight == code).sum()) for name, code in (("WEIGHTED", mo.WEIGHTED), ("LAST_VERTEX", mo.LAST_VERTEX), ("BACK_SIDE", mo.BACK_SIDE))}
    for t in (1, 2):
        out["weighted on type %d" % t] = int(((weight == mo.WEIGHTED) & (mtype == t)[:, :, None]).sum())
    for c in (0, 1, 2):
        out["later hit, count %d" % c] = int((count == c).sum())
    assert (count[:, 0] == -1).all() and np.all((wb >= 0.0) & (wb <= 1.0))
    assert np.all(wb[count == 0] == 1.0)                          # an emitter the list does not name: the BRDF ray carries all of it
    return out


@pytest.mark.parametrize("K,B", mc.SEARCH_KB + (mc.LIST_KB,))
def test_the_cornell_box_reaches_every_weight_rule(K, B):
    """40 x 24, 3 frames, the emitters' list.  Measured at (K 1, B 16; the first eight vertices) / (4, 4) / (2, 4): WEIGHTED 5987 /
    13414 / 6786, LAST_VERTEX - / 3497 / 1740, BACK_SIDE 1388 / 3076 / 1520 (a vertex that sees the light from its back: the ceiling
    beside it), weighted on diffuse 5324 / 11844 / 6024 and on GGX vertices 663 / 1570 / 762, later hits on the light (count 1) 48 /
    29 / 15."""
    e = _edges("cornell", None, K, B)
    print(K, B, e)
    for k in ("WEIGHTED", "LAST_VERTEX", "BACK_SIDE", "weighted on type 1", "weighted on type 2", "later hit, count 1"):
        if k == "LAST_VERTEX" and B > mo.DETAIL_VERTICES:
            continue   # (details reports the first eight vertices; the B = 4 cases cover the rule)
        assert e[k] >= 10, (k, e)
    assert e["later hit, count 0"] == 0 and e["later hit, count 2"] == 0


def test_the_lists_reach_every_count():
    """The five lists at K 2, B 4: a later hit on an emitter reads counts of 1 (every list), 0 (the emitter ``missing`` leaves out)
    and 2 (``duplicated`` and ``unsorted`` name triangle 10 twice).  Such hits are rare at this size -- 15 of 2 880 samples -- and
    every one is compared.  Measured later hits, count 0 / 1 / 2: emitters 0 / 15 / 0, duplicated 0 / 6 / 9, missing 6 / 9 / 0, wall
    0 / 15 / 0, unsorted 0 / 6 / 9; WEIGHTED 6657 .. 6839, BACK_SIDE 1060 .. 1520, LAST_VERTEX 1653 .. 1740."""
    K, B = mc.LIST_KB
    got = {name: _edges("cornell", name, K, B) for name in mc.LISTS}
    for name, e in got.items():
        print(name, e)
        assert e["WEIGHTED"] >= 1000 and e["BACK_SIDE"] >= 100 and e["LAST_VERTEX"] >= 100, (name, e)
        assert e["later hit, count 1"] >= 5, (name, e)
    assert got["missing"]["later hit, count 0"] >= 5
    assert got["duplicated"]["later hit, count 2"] >= 5 and got["unsorted"]["later hit, count 2"] >= 5
    # the clamped list [0, 10, 35, 11]: two walls, both emitters once
    e = _edges("cornell", "clamped", K, B)
    assert e["WEIGHTED"] >= 1000 and e["later hit, count 1"] >= 5, e


def test_the_other_scenes_weigh_light_samples_and_hit_lights_later():
    """finite:5, finite:8 (K 2, B 6: every vertex a GGX one, of every finite roughness; few paths reach the sixth vertex, and few BRDF
    rays the light), nested:10 and nested:15 (K 2, B 4).  Measured WEIGHTED / LAST_VERTEX / BACK_SIDE / later hits: finite:5 4119 /
    0 / 946 / 7, finite:8 4520 / 6 / 806 / 0, nested:10 5723 / 1133 / 1063 / 13, nested:15 5391 / 1166 / 1699 / 6."""
    for name, K, B in mc.FINITE + mc.BIG:
        e = _edges(name, None, K, B)
        print(name, e)
        assert e["WEIGHTED"] >= 1000 and e["BACK_SIDE"] >= 100, (name, e)
        if name.startswith("finite"):
            assert e["weighted on type 2"] == e["WEIGHTED"], (name, e)
        else:
            assert e["LAST_VERTEX"] >= 100 and e["later hit, count 1"] >= 5 and e["weighted on type 2"] >= 100, (name, e)


def test_light_counts_is_the_bincount_of_the_clamped_list():
    assert mo.light_counts([-1, 10, 41, 11], 36).tolist() == np.bincount([0, 10, 35, 11], minlength=36).tolist()
    assert mo.light_counts(NONE, 36).tolist() == [0] * 36 and len(mo.light_counts([3], 0)) == 0
