"""Russian roulette on the CPU: the restatement (tests/roulette_oracle.c) against the restatements it extends, its statistics, and the
proof that every input of tests/test_gpu_roulette.py reaches the edge it is rendered for.  No GPU.

  - identity: first_bounce >= max_bounces plays no roulette and draws no uniform: the framebuffer and every sample's radiance are
    indirect_oracle's / mis_oracle's / power_oracle's, bit for bit;
  - unbiasedness: 16 x 16 Cornell box, B = 8, K = 1, N = 3 200 frames (tests/test_mis_cpu.py's N): the image mean with roulette on
    frames [N, 2N) against the mean without on frames [0, N), per channel within 4 combined standard errors, each standard error from
    its own run's N per-frame image means (frames are independent).  Plain and MIS -- with MIS the rule that pb is NOT scaled by q is
    what is under test.  Measured |difference| in standard errors per channel: plain R 1 cap 0.95: 1.04 1.02 1.00; plain R 3 cap 0.5:
    1.02 1.05 0.99; MIS R 1 cap 0.95: 1.00 1.00 1.00; MIS R 3 cap 0.5: 0.99 1.03 0.99.  All are 1.0 for one reason: frames [N, 2N) hold
    ONE sample of radiance 375 730 (a light sample of the parent estimator at a first vertex close under the light, with or without
    roulette), which alone makes both the difference of the means (0.46) and its standard error (0.46).  The check is the one the
    estimator's statement asks for and it holds, but such a tail leaves it little power, so a sharper one stands beside it:
  - unbiasedness, sample by sample: on the SAME frames a sample with and one without roulette share their seed and everything up to
    the first roulette, that tail among it; the mean of the N per-frame differences lies within 4 of its own standard errors.
    Measured |mean| / standard error per channel: plain R 1 cap 0.95: 1.34 1.10 1.35 (standard error 0.041 0.029 0.004 on means of
    1.43 1.34 1.02); plain R 3 cap 0.5: 0.96 1.54 0.59; MIS R 1 cap 0.95: 0.63 0.62 0.03 (standard error 0.004 0.003 0.001); MIS R 3
    cap 0.5: 1.32 0.07 0.46;
  - path lengths: with roulette the mean number of vertices per path is lower than without, on the same frames (asserted); the ratio
    of the variances per sample is printed (recorded in DESIGN.md S4, not asserted).  Measured, same setup: vertices 4.29 without,
    2.12 (R 1, cap 0.95) and 2.59 (R 3, cap 0.5) with; variance per sample x 5.65 and x 0.93 (plain), x 1.11 and x 1.09 (MIS);
  - edges: roulette_cases.EDGES, each reached at least once by the scene and size the device renders."""
import numpy as np
import pytest

import indirect_oracle as io
import mis_oracle as mo
import power_oracle as po
import roulette_cases as rc
import roulette_oracle as ro
from conftest import assert_fb_equal
from scenes import edge_scene


# ---- identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,B", [("cornell", 2, 6), ("finite:5", 1, 4), ("nested:15", 1, 3)])
@pytest.mark.parametrize("R", ["B", ro.NEVER])
def test_no_roulette_is_the_parent_restatement(name, K, B, R):
    tris, mats, lights, cam = edge_scene(name)[1]
    Ws, Hs, F = 16, 12, 2
    R = B if R == "B" else R
    gid, frame = io.all_samples(Ws, Hs, F)
    parents = {(False, False): (io.render(tris, mats, Ws, Hs, 0, F, K, B, lights=lights, cam=cam), io.samples(tris, mats, Ws, Hs, gid, frame, K, B, lights=lights, cam=cam)[0]),
               (True, False): (mo.render(tris, mats, Ws, Hs, 0, F, K, B, lights=lights, cam=cam), mo.samples(tris, mats, Ws, Hs, gid, frame, K, B, lights=lights, cam=cam)[0]),
               (False, True): (po.render(po.INDIRECT, tris, mats, Ws, Hs, 0, F, K, B, lights=lights, cam=cam), po.samples(po.INDIRECT, tris, mats, Ws, Hs, gid, frame, K, B, lights=lights, cam=cam)),
               (True, True): (po.render(po.MIS, tris, mats, Ws, Hs, 0, F, K, B, lights=lights, cam=cam), po.samples(po.MIS, tris, mats, Ws, Hs, gid, frame, K, B, lights=lights, cam=cam))}
    for (mis, power), (want_fb, want_rad) in parents.items():
        what = "%s R %d mis %d power %d" % (name, R, mis, power)
        assert_fb_equal(ro.render(tris, mats, Ws, Hs, 0, F, K, B, R, 0.25, mis=mis, power=power, lights=lights, cam=cam), want_fb, what)
        rad, vertices, end, code, s, q, r = ro.samples(tris, mats, Ws, Hs, gid, frame, K, B, R, 0.25, mis=mis, power=power, lights=lights, cam=cam, details=True)
        assert_fb_equal(rad, want_rad, what + ": radiance before the fold")
        assert (code == ro.RR_NONE).all() and (end[:, 0] != ro.END_ROULETTE).all(), what


def test_the_account_is_consistent():
    """the roulette's account agrees with itself and with the estimator's statement, sample by sample"""
    tris, mats, lights, cam = edge_scene("cornell")[1]
    gid, frame = io.all_samples(24, 16, 3)
    B, R, cap = 6, 2, np.float32(0.5)
    rad, vertices, end, code, s, q, r = ro.samples(tris, mats, 24, 16, gid, frame, 1, B, R, cap, mis=True, details=True)
    played = code != ro.RR_NONE
    assert not played[:, :R - 1].any() and not played[:, B - 1].any(), "played before R or at the last vertex"
    with np.errstate(invalid="ignore"):
        assert np.array_equal(q[played], np.where(cap < s[played], cap, s[played]).astype(np.float32))
        assert (q[code == ro.RR_PASS] >= 1.0).all() and (r[code == ro.RR_SURVIVED] < q[code == ro.RR_SURVIVED]).all()
        assert not (r[code == ro.RR_ENDED] < q[code == ro.RR_ENDED]).any()
    ended = end[:, 0] == ro.END_ROULETTE
    assert ended.any() and np.array_equal((code == ro.RR_ENDED).sum(axis=1), ended.astype(int))
    assert (code[ended, end[ended, 1]] == ro.RR_ENDED).all() and np.array_equal(vertices[ended], end[ended, 1] + 1)


# ---- the statistics ------------------------------------------------------------------------------------------------------------
N, SW, SH, SK, SB = 3200, 16, 16, 1, 8
SETTINGS = [(1, 0.95), (3, 0.5)]
_RUNS = {}


def _run(mis, R, cap, frame_begin):
    k = (mis, R, cap, frame_begin)
    if k not in _RUNS:
        tris, mats = edge_scene("cornell")[1][:2]
        _RUNS[k] = ro.sample_frames(tris, mats, SW, SH, N, SK, SB, R, cap, mis=mis, frame_begin=frame_begin)
    return _RUNS[k]


def _mean_se(rad):
    per_frame = rad.mean(axis=1)
    return per_frame.mean(axis=0), per_frame.std(axis=0, ddof=1) / np.sqrt(len(per_frame))


@pytest.mark.parametrize("mis", [False, True], ids=["plain", "mis"])
@pytest.mark.parametrize("R,cap", SETTINGS)
def test_roulette_is_unbiased(mis, R, cap):
    (ma, sa), (mb, sb) = _mean_se(_run(mis, R, cap, N)[0]), _mean_se(_run(mis, ro.NEVER, 1.0, 0)[0])
    z = np.abs(ma - mb) / np.sqrt(sa ** 2 + sb ** 2)
    print("mis %d R %d cap %g: means %s against %s, |difference| in standard errors per channel %s" % (mis, R, cap, ma, mb, z))
    assert (z <= 4.0).all(), z


@pytest.mark.parametrize("mis", [False, True], ids=["plain", "mis"])
@pytest.mark.parametrize("R,cap", SETTINGS)
def test_roulette_shortens_the_paths(mis, R, cap):
    """on the same samples (frames [0, N)): fewer vertices per path; the variance per sample's ratio is printed, not asserted"""
    rad, vertices, end = _run(mis, R, cap, 0)
    rad0, vertices0, end0 = _run(mis, ro.NEVER, 1.0, 0)
    var, var0 = rad.var(axis=0, ddof=1).mean(), rad0.var(axis=0, ddof=1).mean()
    print("mis %d R %d cap %g: vertices per path %.3f against %.3f; ended by roulette %.1f %%; variance per sample %.4g against %.4g (x %.3f)"
          % (mis, R, cap, vertices.mean(), vertices0.mean(), 100.0 * (end == ro.END_ROULETTE).mean(), var, var0, var / var0))
    assert (end0 != ro.END_ROULETTE).all() and (end == ro.END_ROULETTE).any()
    assert vertices.mean() < vertices0.mean()


@pytest.mark.parametrize("mis", [False, True], ids=["plain", "mis"])
@pytest.mark.parametrize("R,cap", SETTINGS)
def test_roulette_is_unbiased_sample_by_sample(mis, R, cap):
    """A sharper form of the check above, on the SAME frames [0, N): a sample with and without roulette shares its seed, so everything up
    to the first roulette -- the parent's rare, very large light samples at the first vertices among it -- is the same in both and
    cancels in the difference.  The N per-frame means of the differences are independent and have expectation 0: their mean lies within
    4 of their own standard errors."""
    d = (_run(mis, R, cap, 0)[0] - _run(mis, ro.NEVER, 1.0, 0)[0]).mean(axis=1)
    m, se = d.mean(axis=0), d.std(axis=0, ddof=1) / np.sqrt(len(d))
    print("mis %d R %d cap %g: mean difference %s, standard error %s, ratio %s" % (mis, R, cap, m, se, np.abs(m) / se))
    assert (np.abs(m) <= 4.0 * se).all(), (m, se)


# ---- every edge the device renders is reached ----------------------------------------------------------------------------------
def _edge(edge):
    name, Ws, Hs, frames, K, B, R, cap, mis = rc.EDGES[edge]
    rad, vertices, end, code, s, q, r = rc.edge_details(edge)
    return B, R, np.float32(cap), rad, vertices, end, code, s, q, r


def test_edge_q_at_least_one():
    B, R, cap, rad, vertices, end, code, s, q, r = _edge("q_at_least_one")
    hit = code == ro.RR_PASS
    assert hit.sum() >= 10 and (s[hit] >= 1.0).all() and (s[hit] > 1.0).any(), "no glossy mask above 1"


def test_edge_capped():
    B, R, cap, rad, vertices, end, code, s, q, r = _edge("capped")
    hit = (code != ro.RR_NONE) & (s > cap)
    assert hit.sum() >= 100 and (q[hit] == cap).all() and cap < 1.0
    assert (code[hit] == ro.RR_SURVIVED).any() and (code[hit] == ro.RR_ENDED).any()


def test_edge_nan_mask():
    B, R, cap, rad, vertices, end, code, s, q, r = _edge("nan_mask")
    hit = (code != ro.RR_NONE) & np.isnan(q)
    assert hit.sum() >= 3, "no NaN mask reached the roulette"
    assert (code[hit] == ro.RR_ENDED).all(), "a NaN q let a path go on"


def test_edge_nonpositive():
    B, R, cap, rad, vertices, end, code, s, q, r = _edge("nonpositive")
    hit = (code != ro.RR_NONE) & (s <= 0.0)
    assert hit.sum() >= 10 and (code[hit] == ro.RR_ENDED).all()


def test_edge_first_eligible():
    B, R, cap, rad, vertices, end, code, s, q, r = _edge("first_eligible")
    first = (end[:, 0] == ro.END_ROULETTE) & (end[:, 1] == R - 1)
    assert R > 1 and first.sum() >= 10 and not (code[:, :R - 1] != ro.RR_NONE).any()
    assert ((end[:, 0] == ro.END_ROULETTE) & (end[:, 1] > R - 1)).any(), "no path ended by a later roulette"


def test_edge_survivor():
    B, R, cap, rad, vertices, end, code, s, q, r = _edge("survivor")
    full = (vertices == B) & (end[:, 0] == ro.END_DEPTH)
    survived = full & np.isin(code[:, R - 1:B - 1], (ro.RR_SURVIVED, ro.RR_PASS)).all(axis=1) & (code[:, R - 1:B - 1] == ro.RR_SURVIVED).any(axis=1)
    assert survived.sum() >= 10, "no path survived every roulette to the last vertex"


def test_r_equal_to_q_is_not_met():
    """r == q exactly decides a path by the strictness of r < q; the GPU comparison covers it only where the inputs meet it: none does,
    so tests/test_gpu_roulette.py asserts nothing about it"""
    met = 0
    for edge in rc.EDGES:
        code, q, r = rc.edge_details(edge)[3], rc.edge_details(edge)[5], rc.edge_details(edge)[6]
        met += int(((code != ro.RR_NONE) & (r == q)).sum())
    print("samples with r == q over the edge inputs: %d" % met)


def test_every_refill_count_is_one_chunk_of_that_many_items():
    run = rc.rr_run()
    assert run % 64 == 0 and run >= 64
    for n in rc.refill_counts():
        Ws, Hs, frames = rc.refill_shape(n)
        assert Ws * Hs * frames == n and Ws >= 1 and Hs >= 1


def test_the_refill_inputs_end_paths_at_different_vertices():
    """R = 1, cap = 0.25 on the Cornell box: the paths of one run end at every vertex from 0 on, so refills happen mid-run"""
    tris, mats, lights, cam = edge_scene("cornell")[1]
    Ws, Hs, frames = rc.refill_shape(3 * rc.rr_run() + 7)
    gid, frame = io.all_samples(Ws, Hs, frames)
    vertices = ro.samples(tris, mats, Ws, Hs, gid, frame, 1, 8, 1, 0.25)[1]
    assert len(np.unique(vertices[:64])) >= 3 and len(np.unique(vertices)) >= 4, np.bincount(vertices)
    for n in rc.refill_counts()[1:]:
        Ws, Hs, frames = rc.refill_shape(n)
        gid, frame = io.all_samples(Ws, Hs, frames)
        assert len(np.unique(ro.samples(tris, mats, Ws, Hs, gid, frame, 1, 8, 1, 0.25)[1])) >= 3, n
