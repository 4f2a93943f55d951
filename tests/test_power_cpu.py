"""Light choice by power on the CPU: the restatement (tests/power_oracle.c) against hand-made tables, against its parents where
they must agree, on the edges the GPU modules render, and as an estimator -- unbiased against the uniform choice, and with the variance
gain DESIGN.md S4 states.  The inputs of tests/test_gpu_light_scale.py are proved here to be what they are for: lists of 524 289 and
2^24 - 1 entries whose table passes 2^32 inside a tile, has 257 tiles, and is read by the renders at entries above 2^16 and 2^23 and
at counts above 2^15; and power_scenes.power_sweep, whose quanta are checked against numpy's float32 arithmetic and whose q = 0 entries
against causes found in float64 from the scene alone.  No GPU."""
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


# ---- reachability: the long lists (tests/test_gpu_light_scale.py renders them) ---------------------------------------------------
TILE = 2048   # csrc/pt_kernels.h: PT_LIGHT_SCAN_TILE
LW, LH = pc.W, pc.H
# measured at 40 x 24, K 4, B 4 on "long" (3 frames): light samples whose entry has cdf[entry] >= 2^32: 4597 (direct) / 12783 / 12783,
# whose entry is >= 2^16: 7241 / 20048 / 20048, whose entry follows a q = 0 one: 103 / 249 / 249.  On "max" (2 frames): entries >= 2^23:
# 2788 / 7613 / 7613; on "panels": 2788 / 7612 / 7612.  The floors are half of that.
_LONG_FLOORS = {po.DIRECT: (2298, 3620, 51), po.INDIRECT: (6391, 10024, 124), po.MIS: (6391, 10024, 124)}
_MAX_FLOORS = {po.DIRECT: 1394, po.INDIRECT: 3806, po.MIS: 3806}


def test_the_long_list_passes_two_to_the_32_inside_a_tile():
    """total 9 692 185 602, which binary32 cannot hold; 257 tiles; the running sum passes 2^32 at entry 232 375, the 952nd of its tile;
    143 tiles start at or above 2^32 (the floor: half)"""
    cdf, tri_q, counts = pc.table_of("unequal", "long")
    total = int(cdf[-1])
    assert len(cdf) == ps.LONG + 1 and total >= 1 << 32 and int(np.float32(total)) != total
    offsets = cdf[:-1:TILE]                                           # what pt_light_tiles_kernel leaves in tile_sums
    assert len(offsets) == 257
    first = int(np.searchsorted(cdf, 1 << 32)) - 1                    # the entry whose q carries the sum over 2^32
    assert 0 < first % TILE < TILE - 1 and int(cdf[first]) < 1 << 32 < int(cdf[first + 1])
    assert int((offsets >= 1 << 32).sum()) >= 71
    qs = np.diff(cdf.astype(np.int64))
    assert (qs == 0).any() and (qs == 1).any() and (qs == 65536).sum() > ps.LONG // 5 and int(counts.max()) >= 1 << 15


@pytest.mark.parametrize("mode", pc.MODES, ids=[pc.MODE_NAMES[m] for m in pc.MODES])
def test_the_long_list_is_read_above_two_to_the_32(mode):
    """the choice reads cdf values of more than 32 bits, entries above 2^16 (a search of more than 16 levels) and entries behind a q = 0
    one; the MIS estimator's later hits read counts of 75 354"""
    (rad, entry, q, reason, later), li = pc.details(mode, "unequal", "long", LW, LH, pc.FRAMES, *pc.LONG_KB)
    cdf = pc.table_of("unequal", "long")[0]
    qs = np.diff(cdf.astype(np.int64))
    chosen = entry[entry >= 0].astype(np.int64)
    wide, far, behind = _LONG_FLOORS[mode]
    assert (qs[chosen] > 0).all() and (q[entry >= 0] == qs[chosen]).all()
    assert int((cdf[chosen] >= 1 << 32).sum()) >= wide and int((chosen >= 1 << 16).sum()) >= far
    assert int((qs[chosen[chosen > 0] - 1] == 0).sum()) >= behind
    assert not np.isnan(rad).any()
    if mode == po.MIS:
        assert int(later.max()) >= 1 << 15                            # (measured 75 354)
    assert not np.isnan(pc.wanted_uniform(mode, "unequal", "long", LW, LH, pc.FRAMES, *pc.LONG_KB)[1]).any()


@pytest.mark.parametrize("mode", pc.MODES, ids=[pc.MODE_NAMES[m] for m in pc.MODES])
@pytest.mark.parametrize("name", ["max", "panels"])
def test_the_longest_lists_are_read_above_two_to_the_23(mode, name):
    (rad, entry, q, reason, later), li = pc.details(mode, "unequal", name, LW, LH, pc.MAX_FRAMES, *pc.LONG_KB)
    assert len(li) == ps.MAX == (1 << 24) - 1
    assert int((entry >= 1 << 23).sum()) >= _MAX_FLOORS[mode] and not np.isnan(rad).any()


def test_the_all_panel_list_has_the_largest_total_the_abi_admits():
    cdf = pc.table_of("unequal", "panels")[0]
    assert int(cdf[-1]) == (1 << 40) - 65536 and (np.diff(cdf) == 65536).all()
    assert ((1 << 24) - 1) * int(cdf[-1]) < 1 << 64                   # the largest u times the largest total: pt_light_table_inv's product
    total = int(pc.table_of("unequal", "max")[0][-1])
    assert total >= 1 << 32 and int(np.float32(total)) != total      # (310 454 888 398)


# ---- reachability: the numeric domain of the table's powers and quanta (power_scenes.power_sweep) -------------------------------
FLT_MAX, FLT_MIN, FLT_TRUE_MIN = float(np.finfo(np.float32).max), 2.0 ** -126, 2.0 ** -149


def _f32_fma(a, b, c):
    """fma on float32 arrays through float64: the product is exact there, the sum is rounded to 53 bits and then to 24 -- the fused
    result except where the 53-bit sum falls on a tie of binary32, which none of these inputs does (the tables below would differ)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _sweep_power32(tris, mats):
    """p_i of every triangle in numpy's float32 arithmetic: include/pt_shim.h's expressions, a second opinion on power_oracle.c"""
    with np.errstate(all="ignore"):
        p1, p2, p3 = (tris[k][:, :3] for k in ("p1", "p2", "p3"))
        a, b = p3 - p1, p2 - p1                                       # N = cross(e2, e1)
        N = [_f32_fma(a[:, i], b[:, j], -(a[:, j] * b[:, i])) for i, j in ((1, 2), (2, 0), (0, 1))]
        n2 = _f32_fma(N[2], N[2], _f32_fma(N[1], N[1], N[0] * N[0]))
        area = np.float32(0.5) * np.sqrt(n2)
        em = mats["emissive"][np.clip(tris["id"], 0, len(mats) - 1)]
        pw = area * ((em[:, 0] + em[:, 1]) + em[:, 2])
        assert pw.dtype == np.float32
        return np.where((pw > 0) & (pw < np.inf), pw, np.float32(0))


def _sweep_tables():
    tris, mats, lists = ps.power_sweep()
    return {name: po.table(tris, mats, li) for name, li in lists.items()}


def test_the_sweeps_quanta_are_numpys():
    """every q of every list: floor(pw / pmax x 65536) in float32, at least 1 where pw > 0; and tri_q the q of the entries that name the
    triangle"""
    tris, mats, lists = ps.power_sweep()
    pw32 = _sweep_power32(tris, mats)
    for name, (cdf, tri_q) in _sweep_tables().items():
        j = np.clip(lists[name], 0, len(tris) - 1)
        p = pw32[j]
        with np.errstate(all="ignore"):
            q = np.floor((p / p.max()) * np.float32(65536.0)).astype(np.int64) if p.max() > 0 else np.zeros(len(p), np.int64)
        q = np.where(p > 0, np.maximum(q, 1), 0)
        assert np.array_equal(np.diff(cdf.astype(np.int64)), q), name
        want = np.zeros(len(tris), np.int64)
        want[j] = q
        assert np.array_equal(tri_q, want), name


def test_the_sweep_covers_the_quantum():
    """over all lists: 3567 entries with 1 < q < 65536, 1601 distinct q, 599 entries whose q is a power of two other than 1 and 65536;
    3126 q = 1 entries of positive power whose quotient pw / pmax is subnormal or zero; the list "subnormal" has
    a subnormal pmax and 90 entries with 1 < q < 65536; "zeros" has 602 entries.  The floors: 2000, 500 and 32 as the scene was
    specified; half the measured otherwise"""
    tris, mats, lists = ps.power_sweep()
    pw32 = _sweep_power32(tris, mats)
    tables = _sweep_tables()
    qs = np.concatenate([np.diff(cdf.astype(np.int64)) for cdf, _ in tables.values()])
    mid = qs[(qs > 1) & (qs < 65536)]
    print("1 < q < 65536:", len(mid), "distinct q:", len(np.unique(qs)), "powers of two:", int((mid & (mid - 1) == 0).sum()))
    assert len(mid) >= 2000 and len(np.unique(qs)) >= 500 and int((mid & (mid - 1) == 0).sum()) >= 32
    underflowed = 0
    for name, (cdf, _) in tables.items():
        p = pw32[np.clip(lists[name], 0, len(tris) - 1)]
        with np.errstate(all="ignore"):
            quotient = p / p.max() if p.max() > 0 else np.ones_like(p)
        low = (p > 0) & (quotient < np.float32(FLT_MIN))
        assert (np.diff(cdf.astype(np.int64))[low] == 1).all(), name
        underflowed += int(low.sum())
    print("q = 1 through a subnormal or zero quotient:", underflowed)
    assert underflowed >= 1563
    p = pw32[lists["subnormal"]]
    q = np.diff(tables["subnormal"][0].astype(np.int64))
    print("the subnormal list: pmax", p.max(), "1 < q < 65536:", int(((q > 1) & (q < 65536)).sum()))
    assert 0 < p.max() < np.float32(FLT_MIN) and int(((q > 1) & (q < 65536)).sum()) >= 45
    assert pw32[np.clip(lists["floor"], 0, len(tris) - 1)].max() > 2.0 ** 120
    assert (np.diff(tables["zeros"][0]) == 0).all() and int(tables["zeros"][0][-1]) == 0 and len(lists["zeros"]) >= 301
    assert lists["all"].min() < 0 and lists["all"].max() >= len(tris) and set(range(len(tris))) <= set(np.clip(lists["all"], 0, len(tris) - 1).tolist())


# measured: the triangles named by some list whose q is 0 there for each cause, found in float64 from the scene alone.  The floors: half
# (measured: 45, 60, 49, 144, 47, 32, 60, 214)
_CAUSES = {"nan": 22, "infinity": 30, "overflowed sum": 24, "overflowed area": 72, "negative sum": 23, "zero area": 16, "zero emission": 30,
           "underflowed area": 107}


def _sweep_causes(tris, mats):
    """{cause: bool [ntri]}: why a triangle has no positive finite power, from the records in float64 -- nothing of the restatement"""
    em = mats["emissive"][np.clip(tris["id"], 0, len(mats) - 1), :3].astype(np.float64)
    p1, p2, p3 = (tris[k][:, :3].astype(np.float64) for k in ("p1", "p2", "p3"))
    with np.errstate(all="ignore"):
        n2 = (np.cross(p3 - p1, p2 - p1) ** 2).sum(axis=1)
        s = em.sum(axis=1)
    finite = np.isfinite(em).all(axis=1)
    lit = finite & (s > 0) & (s <= FLT_MAX)                          # a positive finite emission sum (exact in float64)
    return {"nan": np.isnan(em).any(axis=1), "infinity": np.isinf(em).any(axis=1) & ~np.isnan(em).any(axis=1),
            "overflowed sum": finite & (s > 1.5 * FLT_MAX), "negative sum": finite & (s < 0), "zero emission": (em == 0).all(axis=1),
            "zero area": lit & (n2 == 0), "overflowed area": lit & (n2 > 4 * FLT_MAX),
            "underflowed area": lit & (n2 > 0) & (n2 < FLT_TRUE_MIN / 4)}, n2


def test_the_sweep_reaches_every_cause_of_q_zero_and_both_ends_of_the_square_roots_window():
    """triangles without power, by cause (float64, from the scene alone): NaN 45, infinity 60, an overflowed sum 49, an overflowed area
    144, a negative sum 47, no area 32, no emission 60, an underflowed area 214 -- the restatement gives each q = 0, and 3348 others a
    q > 0; dot(N, N) within a factor 4 below / above 1e-30: 17 / 31, of 1e30: 20 / 10, subnormal: 286.  The floors are half of that"""
    tris, mats, lists = ps.power_sweep()
    causes, n2 = _sweep_causes(tris, mats)
    tri_q = _sweep_tables()["all"][1]                                # every triangle is named by "all"
    for name, floor in _CAUSES.items():
        print(name, int(causes[name].sum()))
        assert int(causes[name].sum()) >= floor, name
        assert (tri_q[causes[name]] == 0).all(), name
    assert int((tri_q > 0).sum()) >= 2000                            # (measured 3348) and the rest has a power
    # dot(N, N) within a factor 4 below and above each end of pt_sqrt's window, and in the subnormals: measured 17, 31, 20, 10 and 286
    near = [int(((n2 >= lo) & (n2 < hi)).sum()) for lo, hi in ((0.25e-30, 1e-30), (1e-30, 4e-30), (0.25e30, 1e30), (1e30, 4e30),
                                                                 (FLT_TRUE_MIN, FLT_MIN))]
    print("dot(N, N) about 1e-30, about 1e30, subnormal:", near)
    assert all(n >= f for n, f in zip(near, (8, 15, 10, 5, 143))), near
    ids = tris["id"]
    assert (ids < 0).sum() >= 32 and (ids >= len(mats)).sum() >= 32   # material indices clamped at both ends
    flat = np.arange(len(tris)) % 2 == 0
    assert (tris["p1"][flat, :3] == 0).all() and (np.abs(tris["p1"][~flat, :3]) > 0).all()


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
