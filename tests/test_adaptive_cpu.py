"""Adaptive sampling on the CPU: the restatement (tests/adaptive_oracle.py) against the rule worked by hand, and the proof that the
inputs of tests/test_gpu_adaptive.py (tests/adaptive_cases.py) reach the loop's edges -- partial lists about a wave and about a run of
the refilling kernel, pixels that stop at once and pixels that run to the cap.  No device."""
from fractions import Fraction

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_oracle as ao
import moments_oracle as mom
import roulette_cases as rc


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_made_records():
    m, want, what = ac.hand_records()
    got, taken = ao.active(m, ac.RULE)
    for i, name in enumerate(what):
        assert got[i] == want[i], name
    assert [int(t) for t in taken] == [int(a) + int(b) for a, b in zip(m["n"], m["rejected"])], "taken is formed in 64 bits"
    assert taken[what.index("n + rejected passes 2^32")] == (1 << 32) + 1
    slots = ao.select(m, ac.RULE)
    assert np.array_equal(slots["pixel"], np.flatnonzero(want)) and np.all(np.diff(slots["pixel"].astype(np.int64)) > 0)
    assert np.array_equal(slots["frame"], (m["n"] + m["rejected"])[want]), "frame = (uint32)taken"
    raw = ao.list_bytes(m, ac.RULE)
    assert np.frombuffer(raw[:16], np.uint32).tolist() == [int(want.sum()), 0, 0, 0] and len(raw) == 16 + 8 * int(want.sum())


def test_the_boundary_record_sits_on_the_boundary_exactly():
    """in exact arithmetic: b == tol2 * (c + floor2) for the boundary record, and above it for its neighbour"""
    m, _, what = ac.hand_records()
    for name, above in (("b == tol2 * (c + floor2) exactly", False), ("b just above the boundary", True)):
        r = m[what.index(name)]
        n, s, s2 = int(r["n"]), Fraction(float(r["sum"][0])), Fraction(float(r["sum2"][0]))
        b = (s2 - s * s / n) / (n - 1) / n
        c = (s / n) ** 2
        bound = Fraction(ac.RULE.tol2) * (c + Fraction(ac.RULE.floor2))
        assert (b > bound) == above and (above or b == bound), name
        fb, fc = ao.terms(m[what.index(name): what.index(name) + 1])
        assert Fraction(float(fb[0])) == b or above, "the restatement's b is exact for the boundary record"
        assert Fraction(float(fc[0])) == c


def test_terms_are_the_summary_s_terms():
    """b and c summed by the fixed tree are se2_sum and mean2_sum of pt_moments_resolve's restatement"""
    rng = np.random.default_rng(3)
    s = rng.uniform(0, 4, (9, 130, 3)).astype(np.float32)
    m = mom.accumulate(s)
    b, c = ao.terms(m)
    want = mom.summary(m)
    assert mom.tree_sum(b) == want["se2_sum"] and mom.tree_sum(c) == want["mean2_sum"]


def test_rule_of_squares_in_python_floats():
    assert ao.rule_of(0.1, 1e-2, 8, 40) == (0.1 * 0.1, 1e-2 * 1e-2, 8, 40)


@pytest.mark.parametrize("pattern", ac.PATTERNS)
def test_select_records_have_the_pattern_they_name(pattern):
    for pixels in ac.select_sizes():
        m, want = ac.select_records(pixels, pattern)
        got, _ = ao.active(m, ac.RULE)
        assert np.array_equal(got, want), (pixels, pattern)
        if pattern == "seeded" and pixels > 64:
            assert 0 < want.sum() < pixels
    t = ac.scan_tile()
    assert ac.select_sizes() == [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]


# ---- the loop's inputs reach their edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.LOOPS))
def test_the_loop_cases_reach_the_edges(name):
    scene, W, H, K, B, R, cap, mis, kw = ac.LOOPS[name]
    L = ac.loop(name)
    npix, fpp, run = W * H, kw["frames_per_pass"], rc.rr_run()
    assert len(L.passes) >= 3 and all(0 < n < npix for n in L.passes), L.passes        # partial lists in every pass
    assert all(a > b for a, b in zip(L.passes, L.passes[1:])), L.passes                   # the lists shrink
    items = [n * fpp for n in L.passes]
    assert min(items) < 64 < max(items) and min(items) < run < max(items), items     # both sides of a wave and of a run
    assert any(n % 64 for n in items), items
    values = np.unique(L.counts)
    assert len(values) >= 4, values
    assert (L.counts == kw["min_samples"]).any() and (L.counts >= kw["max_samples"]).any()
    assert int(L.counts.max()) < kw["max_samples"] + fpp
    assert L.finite and int(L.moments["rejected"].sum()) == 0
    assert int(L.counts.sum()) == npix * kw["min_samples"] + sum(items)
    assert not ao.active(L.moments, ao.rule_of(kw["tolerance"], kw["floor"], kw["min_samples"], kw["max_samples"]))[0].any()


def test_the_lbvh_case_takes_the_lbvh():
    from scenes import edge_scene

    assert len(edge_scene(ac.LOOPS["lbvh_mis"][0])[1][0]) >= 512


def test_a_pixel_holds_the_uniform_render_of_its_own_frames():
    """the identity the restated image is built on, checked the long way for one case: folding each pixel's own samples in order gives
    the pixel of the uniform render after as many frames"""
    import direct_oracle as do
    import roulette_oracle as ro
    from scenes import edge_scene

    scene, W, H, K, B, R, cap, mis, kw = ac.LOOPS["cornell_mis"]
    tris, mats, lights, cam = edge_scene(scene)[1]
    L = ac.loop("cornell_mis")
    for n in (kw["min_samples"], int(L.counts.max())):
        full = ro.render(tris, mats, W, H, 0, n, K, B, R, cap, mis=mis, lights=lights, cam=cam)
        resumed = ro.render(tris, mats, W, H, kw["min_samples"] - 1, n - kw["min_samples"] + 1, K, B, R, cap, mis=mis, lights=lights, cam=cam,
                            start=ro.render(tris, mats, W, H, 0, kw["min_samples"] - 1, K, B, R, cap, mis=mis, lights=lights, cam=cam))
        assert full.tobytes() == resumed.tobytes()
        sel = L.counts == n
        assert sel.any() and L.fb[sel].tobytes() == full[sel].tobytes()
    assert len(do.local_gids(W, H)) == len(L.counts)
