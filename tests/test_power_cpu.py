"""Light choice by power on the CPU: the restatement (tests/power_oracle.c) against hand-made tables, against its parents where
they must agree, on the edges the GPU module renders, and as an estimator -- unbiased against the uniform choice, and with the variance
gain DESIGN.md S4 states.  No GPU."""
import numpy as np
import pytest

import direct_oracle as do
import indirect_oracle as io
import mis_oracle as mo
import power_cases as pc
import power_oracle as po
import power_scenes as ps
from conftest import assert_fb_equal
from oclpathtracer_amd import scene

NONE = np.zeros(0, np.int32)
W, H, FRAMES = pc.W, pc.H, pc.FRAMES


# ---- the table by hand -----------------------------------------------------------------------------------------------------------
def _kat_scene():
    """triangles: 0 area 0.5, 1 area 1.5, 2 area 0.5, 3 no area, 4 area 0.5 -- materials: 0 emits (1, .5, .5), 1 nothing, 2 emits 2e-5 in
    all, 3 NaN, 4 a sum of -1, 5 infinity"""
    t = np.zeros(5, scene.TRIANGLE_DTYPE)
    for i, (a, b) in enumerate([(1, 1), (1, 3), (1, 1), (0, 0), (1, 1)]):
        t["p1"][i, :3], t["p2"][i, :3], t["p3"][i, :3] = (i, 0, 0), (i + a, 0, 0), (i, b, 0)
    m = np.zeros(6, scene.MATERIAL_DTYPE)
    m["type"] = scene.DIFFUSE
    m["emissive"][0, :3] = (1.0, 0.5, 0.5)
    m["emissive"][2, :3] = (1e-5, 0.5e-5, 0.5e-5)
    m["emissive"][3, :3] = (np.nan, 1.0, 1.0)
    m["emissive"][4, :3] = (1.0, -3.0, 1.0)
    m["emissive"][5, :3] = (np.inf, 0.0, 0.0)
    return t, m


def _table(ids, lights):
    t, m = _kat_scene()
    t = t.copy()
    t["id"] = ids
    cdf, tri_q = po.table(t, m, np.asarray(lights, np.int32))
    return np.diff(cdf.astype(np.int64)).tolist(), int(cdf[-1]), tri_q.tolist()


def test_powers_one_and_three():
    q, total, tri_q = _table([0, 0, 1, 0, 1], [0, 1])
    assert q == [21845, 65536] and total == 87381 and tri_q == [21845, 65536, 0, 0, 0]


def test_a_power_ratio_above_65536_gives_one():
    q, total, tri_q = _table([2, 0, 1, 0, 1], [0, 1])       # 1e-5 against 3
    assert q == [1, 65536] and total == 65537 and tri_q[:2] == [1, 65536]


def test_entries_of_no_power_give_zero():
    # a non-emitter, a light of no area, NaN, a negative sum, infinity; then the two ends of the clamp: -5 -> triangle 0, 99 -> triangle 4
    q, total, tri_q = _table([0, 0, 1, 0, 0], [2, 3, 1, -5, 99, 0, 4])
    assert q == [0, 0, 65536, 21845, 21845, 21845, 21845] and tri_q == [21845, 65536, 0, 0, 21845]
    for ids in ([3, 0, 0, 0, 0], [4, 0, 0, 0, 0], [5, 0, 0, 0, 0]):
        assert _table(ids, [0, 1])[0] == [0, 65536], ids
    q, _, tri_q = _table([99, -7, 1, 1, 1], [0, 1])          # material indices are clamped: 99 -> 5 (infinity), -7 -> 0
    assert q == [0, 65536] and tri_q == [0, 65536, 0, 0, 0]


def test_an_all_zero_list_and_an_empty_one():
    q, total, tri_q = _table([1, 1, 1, 0, 1], [0, 1, 3, 2])
    assert q == [0, 0, 0, 0] and total == 0 and tri_q == [0] * 5
    assert _table([0] * 5, [])[1:] == (0, [0] * 5)


def test_duplicates_share_one_q_and_unnamed_triangles_have_none():
    q, total, tri_q = _table([0, 0, 0, 0, 0], [4, 1, 4, 0, 4])
    assert q == [21845, 65536, 21845, 21845, 21845] and total == 4 * 21845 + 65536 and tri_q == [21845, 65536, 0, 0, 21845]


# ---- the restatement against its parents -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("lights", [(10,), (10, 10), (11, 11, 11, 11)], ids=["nl1", "nl2", "nl4"])
def test_equal_powers_are_the_uniform_choice(cornell, mode, lights):
    """1, 2 or 4 entries of one emitter: inv is nl and the entry floor(u nl / 2^24): the parent restatement's image, bit for bit"""
    tris, mats = cornell
    li, K, B = np.asarray(lights, np.int32), 2, 1 if mode == po.DIRECT else 4
    want = {po.DIRECT: lambda: do.render(tris, mats, W, H, 0, FRAMES, K, lights=li),
            po.INDIRECT: lambda: io.render(tris, mats, W, H, 0, FRAMES, K, B, lights=li),
            po.MIS: lambda: mo.render(tris, mats, W, H, 0, FRAMES, K, B, lights=li)}[mode]()
    assert_fb_equal(po.render(mode, tris, mats, W, H, 0, FRAMES, K, B, lights=li), want, "%s nl %d" % (pc.MODE_NAMES[mode], len(li)))


def test_no_lights_is_the_renderer_and_one_bounce_is_direct(oracle, cornell):
    tris, mats = ps.unequal_lights()
    want = oracle.render(tris, mats, W, H, FRAMES, max_bounces=4)
    for mode in (po.INDIRECT, po.MIS):
        assert_fb_equal(po.render(mode, tris, mats, W, H, 0, FRAMES, 2, 4, lights=NONE), want, "no lights")
        assert_fb_equal(po.render(mode, tris, mats, W, H, 0, FRAMES, 2, 1, lights=ps.edge_list()),
                        po.render(po.DIRECT, tris, mats, W, H, 0, FRAMES, 2, lights=ps.edge_list()), "B = 1")


# ---- reachability: the edges occur on the inputs the GPU module renders for them ------------------------------------------------
# measured on these inputs (40 x 24, 3 frames, K 4, B 4; the edge list): q = 1 entries chosen 8 (direct) / 18 / 18, the first entry
# 2772 / 7562 / 7562, the last 2745 / 7554 / 7554, the entry after the q = 0 wall 2750 / 7691 / 7691; MIS later hits with a count of 1:
# 16, of 2: 16.  The floors are half of that.
_FLOORS = {po.DIRECT: (4, 1300), po.INDIRECT: (9, 3700), po.MIS: (9, 3700)}


@pytest.mark.parametrize("case", [c for c in pc.edge_cases() if c[2] == "edges"], ids=lambda c: pc.MODE_NAMES[c[0]])
def test_the_edge_list_reaches_every_edge_of_the_choice(case):
    (rad, entry, q, reason, later), li = pc.details(*case)
    cdf, tri_q = po.table(*ps.unequal_lights(), li)
    qs = np.diff(cdf.astype(np.int64))
    assert qs[0] == 65536 and qs[1] == 0 and qs[2] == 65536 and qs[-1] == 65536 and qs[-2] == 0 and (qs == 1).sum() == 20 * ps.TINY
    few, many = _FLOORS[case[0]]
    chosen = entry[entry >= 0]
    assert (qs[chosen] > 0).all() and (q[entry >= 0] == qs[chosen]).all()      # an entry of q = 0 is never chosen
    assert int((q == 1).sum()) >= few
    assert int((entry == 0).sum()) >= many and int((entry == len(li) - 1).sum()) >= many and int((entry == 2).sum()) >= many
    assert int((reason == po.EMPTY_TABLE).sum()) == 0 and not np.isnan(rad).any()
    if case[0] == po.MIS:
        assert int((later == 1).sum()) >= 8 and int((later == 2).sum()) >= 8   # tri_q is read at counts of 1 and of 2
    else:
        assert (later == -1).all()


@pytest.mark.parametrize("case", [c for c in pc.edge_cases() if c[2] == "zero"], ids=lambda c: pc.MODE_NAMES[c[0]])
def test_the_zero_list_is_an_empty_table(case):
    """total == 0: every light sample is drawn and none contributes -- measured 8304 (direct) / 22912 of them"""
    (rad, entry, q, reason, later), li = pc.details(*case)
    assert int(po.table(*ps.unequal_lights(), li)[0][-1]) == 0
    drawn = int((reason != do.NOT_DRAWN).sum())
    assert drawn >= (8000 if case[0] == po.DIRECT else 22000) and int((reason == po.EMPTY_TABLE).sum()) == drawn
    assert (entry == -1).all() and not np.isnan(rad).any()
    if case[0] == po.MIS:
        assert int((later == 0).sum()) >= 17 and int((later > 0).sum()) == 0   # (measured 34) the panel, not in the list: wb = 1


def test_every_gpu_input_is_finite():
    for mode in pc.MODES:
        for name in pc.BIG:
            assert not np.isnan(pc.wanted(mode, name, None, W, H, FRAMES, *pc.BIG_KB)[1]).any()


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
# 16 x 16, K = 1, B = 4, N = 3200 frames per estimate: the size of test_mis_cpu's checks.  A standard error is taken from the variance of
# the N per-frame image means (frames are independent; pixels of one frame need not be).
SW = SH = 16
SK, SB, N = 1, 4, 3200
_RAD = {}


def _frames(name, power, mis, frame_begin=0):
    k = (name, power, mis, frame_begin)
    if k not in _RAD:
        tris, mats = ps.unequal_lights() if name == "unequal" else scene.load_model()
        if power:
            assert frame_begin == 0
            _RAD[k] = po.radiance_frames(po.MIS if mis else po.INDIRECT, tris, mats, SW, SH, N, SK, SB)
        else:
            _RAD[k] = mo.radiance_frames(tris, mats, SW, SH, frame_begin, N, SK, SB, mis=mis)
        _RAD[k].setflags(write=False)
    return _RAD[k]


def _variance(rad):
    return float(rad.var(axis=0).mean())   # per pixel and channel over the frames, then the mean


@pytest.mark.parametrize("mis", [False, True], ids=["plain", "mis"])
def test_power_is_unbiased_against_the_uniform_choice(mis):
    """The unequal-lights room, every emitter in the list: power on frames [0, N) against uniform on frames [N, 2N): per channel the
    image means differ by at most 3 standard errors of the difference (measured: -0.97, -0.90, -0.41 plain; -1.01, -0.98, -0.36 MIS)"""
    p, u = _frames("unequal", True, mis).mean(axis=1), _frames("unequal", False, mis, N).mean(axis=1)
    se = np.sqrt(p.var(axis=0, ddof=1) / N + u.var(axis=0, ddof=1) / N)
    z = (p.mean(axis=0) - u.mean(axis=0)) / se
    print("z =", z)
    assert (np.abs(z) <= 3.0).all(), z


@pytest.mark.parametrize("mis,measured", [(False, 459.2), (True, 995.7)], ids=["plain", "mis"])
def test_power_lowers_the_variance_of_unequal_lights(mis, measured):
    """Mean per-pixel variance of the per-sample radiance over frames [0, N), uniform / power on the same frames.  Measured: 459 without
    MIS (4.07e4 against 88.7), 996 with it (4.01e4 against 40.3) -- the uniform choice gives the panel 2 of 59 samples and those a
    weight of 29.5.  The floor is half the measured ratio, the slack for the ratio's own sampling error at this frame count."""
    ratio = _variance(_frames("unequal", False, mis)) / _variance(_frames("unequal", True, mis))
    print("variance ratio uniform / power =", ratio)
    assert ratio > 1.0 and ratio >= measured / 2


@pytest.mark.parametrize("mis", [False, True], ids=["plain", "mis"])
def test_power_changes_nothing_on_equal_lights(mis):
    """The Cornell box alone: two emitters of bit-equal power.  The radiance of every sample is the uniform choice's bit for bit, so the
    two variances are equal exactly -- within any sampling error"""
    p, u = _frames("cornell", True, mis), _frames("cornell", False, mis)
    assert np.array_equal(p, u)
    assert _variance(p) == _variance(u)
