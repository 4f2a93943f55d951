"""Resampled light sampling (pt_render_direct_ris, pt_render_indirect_ris, pt_render_indirect_pixels_ris) on the MI355X, bit for bit.

Every render is compared twice with the restatement (tests/ris_oracle.c), NaN positions equal: the sample workspace with the radiance
before the fold, and the framebuffer.  The inputs are tests/ris_cases.py's -- images of 1, 15, 65 and 40 x 24 pixels, M in {1, 2, 8,
32}, K in {1, 4} and once 256, the brute-force, the tiled and the LBVH kernels, direct and indirect, plain and MIS, the roulette off
and played, B in {1, 2, 8} --; tests/test_ris_cpu.py proves on these very inputs that every edge of the resampling is reached.  The
identities (M = 1 is the parent's image, no lights is the parent's for every M, B = 1 is the direct form) compare the device with
itself."""
import ctypes

import numpy as np
import pytest

import adaptive_support as asup
import direct_oracle as do
import ris_cases as rc
import ris_oracle as rs
from conftest import assert_fb_equal
from gpu_support import SEARCHES, assert_lit_argument_errors, lit_with_samples, options
from oclpathtracer_amd import shim
from oclpathtracer_amd.direct import DirectRenderer
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette
from ris_scenes import ris_scene
from ris_support import RisBuffers, local_pixels

pytestmark = pytest.mark.gpu


def _label(case):
    name, W, H, frames, K, M, B, R, cap, mis = case
    return "%s %dx%dx%d K%d M%d %s" % (name, W, H, frames, K, M, "direct" if B is None else "B%d R%d cap %g mis %d" % (B, R, cap, mis))


def _compare(device, case, what="", **stripes):
    """one raw render of the case against the restatement: the workspace's records, the framebuffer, and nothing behind either"""
    name, W, H, frames = case[:4]
    what = "%s %s" % (what, _label(case))
    want_fb, want_rad = rc.wanted(case, **stripes)
    b = RisBuffers(device, name, W, H, frames=frames)
    try:
        code, fb, ws = b.render_case(case, **stripes)
        assert code == shim.PT_OK, what
        n = local_pixels(W, H, **stripes)
        assert_fb_equal(ws[:frames * n * 3].reshape(frames, n, 3), want_rad, what + ": radiance before the fold")
        assert np.array_equal(ws[frames * n * 3:], b.ws_sentinel[frames * n * 3:]), what + ": the workspace behind the records was written"
        assert_fb_equal(fb[:n], want_fb, what)
        assert np.array_equal(fb[n:], b.sentinel[n:]), what + ": the framebuffer behind the image was written"
    finally:
        b.release()


def _run(device, cases, what, **opts):
    rc.prefetch(cases)
    with options(device, **opts):
        for case in cases:
            _compare(device, case, what)


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------------------
def test_direct_on_the_brute_force_kernel(device):
    _run(device, rc.DIRECT, "direct", ACCEL=1)


def test_direct_with_256_light_samples_of_32_candidates(device):
    _run(device, [rc.DEEP], "K 256", ACCEL=1)


def test_indirect_on_the_refilling_kernel(device):
    """plain and MIS; the roulette off, (1, 0.95) and (3, 0.5); B in {1, 2, 8}; images of 1, 15, 65 and 960 pixels"""
    _run(device, rc.INDIRECT, "indirect", ACCEL=1)


def test_the_tiled_table(device):
    assert 257 <= len(ris_scene("many_tiled")[0]) <= 511
    _run(device, rc.TILED, "tiled", ACCEL=1)


@pytest.mark.parametrize("accel", [0, 2])
def test_the_lbvh(device, accel):
    assert len(ris_scene("many_lbvh")[0]) >= 512
    _run(device, rc.LBVH, "lbvh accel %d" % accel, ACCEL=accel)


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_every_search_option(device, quad, accel):
    _run(device, rc.SEARCH_CASES, "q%d a%d" % (quad, accel), QUAD_FILTER=quad, ACCEL=accel)


@pytest.mark.parametrize("accel", [1, 2])
def test_lists_at_the_edges_of_the_choice(device, accel):
    """edge_list(): q = 0 walls, the emitter of no area, duplicates; zero_list(): a table of total 0; light indices out of range"""
    _run(device, rc.LISTS, "lists accel %d" % accel, ACCEL=accel)


@pytest.mark.parametrize("accel", [1, 2])
def test_vertices_within_the_shadow_rays_offset_of_an_emitter(device, accel):
    """kept candidates with tl <= 0: open, nothing searched"""
    _run(device, rc.NEAR, "near accel %d" % accel, ACCEL=accel)


@pytest.mark.parametrize("accel", [1, 2])
def test_two_frames_in_two_chunks(device, accel):
    """a workspace of one frame: the second chunk overwrites the slot of the first, the framebuffer holds both"""
    with options(device, ACCEL=accel):
        for case in rc.CHUNKED:
            name, W, H, frames = case[:4]
            assert frames == 2
            want_fb, want_rad = rc.wanted(case)
            b = RisBuffers(device, name, W, H, frames=1)
            try:
                code, fb, ws = b.render_case(case)
                assert code == shim.PT_OK
                assert_fb_equal(ws.reshape(1, W * H, 3), want_rad[1:], _label(case) + ": the workspace holds the last chunk's frame")
                assert_fb_equal(fb[:W * H], want_fb, _label(case))
            finally:
                b.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_stripes_over_three_ranks(device, accel):
    with options(device, ACCEL=accel):
        for rank in range(rc.STRIPES["n_ranks"]):
            _compare(device, rc.STRIPED, "rank %d accel %d" % (rank, accel), rank=rank, **rc.STRIPES)


# ---- 2. identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("case", rc.IDENTITY, ids=_label)
def test_one_candidate_is_the_parent_entry_point(device, case, accel):
    """M = 1: workspace and framebuffer of pt_render_direct_power / pt_render_indirect_rr with the table, bit for bit"""
    name, W, H, frames = case[:4]
    b = RisBuffers(device, name, W, H, frames=frames)
    try:
        with options(device, ACCEL=accel):
            code, fb, ws = b.render_case(case)
            pcode, pfb, pws = b.render_case(case, parent=True)
        assert code == pcode == shim.PT_OK
        assert_fb_equal(ws, pws, _label(case) + ": radiance before the fold")
        assert_fb_equal(fb, pfb, _label(case))
        assert not np.array_equal(fb, b.sentinel)
    finally:
        b.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_one_candidate_over_a_list_of_pixels_is_the_parent(device, accel):
    """pt_render_indirect_pixels_ris with M = 1 against pt_render_indirect_pixels on a scattered list; M = 8 against the restatement"""
    name, W, H, _, K, _, B, R, cap, mis = rc.ADAPTIVE
    tris, mats, lights, cam = ris_scene(name)
    F = 2
    slots = asup._scattered(np.random.default_rng(5), W * H, 70)
    b = RisBuffers(device, name, W, H, frames=F)
    try:
        b.estimator(mis, True).set_list(slots)
        p = b.params(b.nl, frame_count=F, light_samples=K, max_bounces=B)
        with options(device, ACCEL=accel):
            got = {}
            for M in (0, 1, 8):   # 0: the parent
                b.reset()
                code = b.call(p, rr=b.roulette(R, cap)) if M == 0 else b.pixels(p, mis=mis, rr=b.roulette(R, cap), ris=b.ris(M))
                assert code == shim.PT_OK, M
                got[M] = (b.read(), b.workspace())
        assert_fb_equal(got[1][1], got[0][1], "M = 1 over a list: radiance before the fold")
        assert_fb_equal(got[1][0], got[0][0], "M = 1 over a list")
        n = F * len(slots) * 3
        gids = do.local_gids(W, H)
        gid = np.tile(gids[slots["pixel"].astype(np.int64)], F)
        frame = (slots["frame"].astype(np.int64)[None, :] + np.arange(F)[:, None]).reshape(-1)
        want = rs.samples(tris, mats, W, H, gid, frame, K, 8, B=B, R=R, cap=cap, mis=mis, lights=lights, cam=cam)
        assert_fb_equal(got[8][1][:n].reshape(-1, 3), want, "M = 8 over a list: radiance before the fold")
        assert np.array_equal(got[8][1][n:], b.ws_sentinel[n:])
        fb = got[8][0].copy()
        assert not np.any(fb[slots["pixel"]] == b.sentinel[0]), "a listed pixel was not folded"
        fb[slots["pixel"]] = b.sentinel[0]
        assert np.array_equal(fb, b.sentinel), "a pixel that is not listed was written"
    finally:
        b.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_no_lights_is_the_parent_for_every_m(device, accel):
    for case in (rc.DIRECT[4], rc.INDIRECT[7]):
        name, W, H, frames = case[:4]
        b = RisBuffers(device, name, W, H, frames=frames)
        try:
            with options(device, ACCEL=accel):
                pcode, pfb, pws = b.render_case(case, parent=True, nl=0)
                assert pcode == shim.PT_OK
                for M in rc.MS:
                    code, fb, ws = b.render_case(case, M=M, nl=0)
                    assert code == shim.PT_OK
                    assert_fb_equal(ws, pws, "%s M %d: radiance before the fold" % (_label(case), M))
                    assert_fb_equal(fb, pfb, "%s M %d" % (_label(case), M))
                # ... through NULL handles of everything that describes the lights
                p = b.direct_params(0) if rc.is_direct(case) else b.params(0, max_bounces=case[6])
                b.reset()
                if rc.is_direct(case):
                    assert b.direct(p, lb=None, qb=None, tq=None) == shim.PT_OK
                else:
                    assert b.indirect(p, mis=True, lb=None, cb=None, qb=None, tq=None) == shim.PT_OK
                assert not np.array_equal(b.read(), b.sentinel)
        finally:
            b.release()


@pytest.mark.parametrize("accel", [1, 2])
@pytest.mark.parametrize("pair", rc.B_ONE, ids=lambda p: "mis%d" % p[0][9])
def test_depth_one_is_the_direct_form(device, pair, accel):
    indirect, direct = pair
    name, W, H, frames = direct[:4]
    b = RisBuffers(device, name, W, H, frames=frames)
    try:
        with options(device, ACCEL=accel):
            icode, ifb, iws = b.render_case(indirect)
            dcode, dfb, dws = b.render_case(direct)
        assert icode == dcode == shim.PT_OK
        assert_fb_equal(iws, dws, "B = 1: radiance before the fold")
        assert_fb_equal(ifb, dfb, "B = 1")
    finally:
        b.release()


# ---- 3. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(device):
    """ris NULL, candidates outside 1 .. 32, a reserved word not 0, cdf or tri_q NULL while num_lights > 0 -- for all three entry points,
    before anything is enqueued --, and the parents' errors through the new entry points"""
    E = shim.PT_ERR_INVALID
    b = RisBuffers(device, "many", 8, 4)
    try:
        b.full_list(32, 0)
        calls = {"direct": (b.direct, b.direct_params(b.nl)), "indirect": (b.indirect, b.params(b.nl)), "pixels": (b.pixels, b.params(b.nl))}
        for what, (call, p) in calls.items():
            assert call(p, ris=None) == E, what
            for M in (0, -1, 33, 1 << 20):
                assert call(p, ris=b.ris(M)) == E, (what, M)
            for k in range(3):
                assert call(p, ris=b.ris(8, reserved=k)) == E, (what, k)
            assert call(p, qb=None) == E and call(p, tq=None) == E and call(p, qb=None, tq=None) == E, what
            assert call(None) == E, what
            assert call(p, lb=None) == E and call(p, sb=None) == E and call(p, fb=None) == E, what
            bad = b.direct_params(b.nl, light_samples=257) if what == "direct" else b.params(b.nl, max_bounces=0)
            assert call(bad) == E, what
            b.assert_untouched()
            assert call(p, ris=b.ris(1)) == shim.PT_OK and call(p, ris=b.ris(32)) == shim.PT_OK, what   # the ends of the range
            b.reset()
        assert b.indirect(b.params(b.nl), rr=None) == E and b.indirect(b.params(b.nl), rr=b.roulette(0, 0.5)) == E
        assert b.indirect(b.params(b.nl), mis=2) == E and b.pixels(b.params(b.nl), pl=None) == E
        assert b.pixels(b.params(b.nl), num_listed=8 * 4 + 1) == E
        b.assert_untouched()
    finally:
        b.release()


class _DirectRis(RisBuffers):
    """RisBuffers whose ``call`` is pt_render_direct_ris, for gpu_support.assert_lit_argument_errors"""

    def params(self, nl, **kw):
        return self.direct_params(nl, **kw)

    def call(self, p, cam=None, **over):
        return self.direct(p, cam=cam, **over)


class _IndirectRis(RisBuffers):
    def call(self, p, cam=None, **over):
        return self.indirect(p, cam=cam, **over)


@pytest.mark.parametrize("cls", [_DirectRis, _IndirectRis])
def test_the_parents_argument_errors(device, cls):
    b = cls(device, "cornell", 16, 8)
    try:
        assert b.nl == 2
        assert_lit_argument_errors(b)
    finally:
        b.release()


# ---- 4. the Python renderers and the adaptive render -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.PYTHON, ids=_label)
def test_python_renderers_against_the_c_abi(device, case):
    name, W, H, frames, K, M, B, R, cap, mis = case
    sc = ris_scene(name)
    kw = dict(light_choice="power", candidates=M)
    if B is not None:
        kw.update(roulette=Roulette(R, cap))
    with options(device, ACCEL=1):
        fb, ws = lit_with_samples(device, sc, W, H, frames, K, max_bounces=B, mis=mis, **kw) if B is not None else \
            lit_with_samples(device, sc, W, H, frames, K, **kw)
        b = RisBuffers(device, name, W, H, frames=frames)
        try:
            code, rfb, rws = b.render_case(case)
        finally:
            b.release()
    assert code == shim.PT_OK
    assert_fb_equal(ws.reshape(-1), rws, _label(case) + ": radiance before the fold")
    assert_fb_equal(fb, rfb[:W * H], _label(case))
    want_fb, _ = rc.wanted(case)
    assert_fb_equal(fb, want_fb, _label(case) + " against the restatement")


def test_python_renderers_refuse_candidates_without_the_table(device):
    tris, mats, _, _ = ris_scene("many")
    for kw in (dict(candidates=2), dict(candidates=2, light_choice="uniform"), dict(candidates=0, light_choice="power"),
               dict(candidates=33, light_choice="power")):
        with pytest.raises(ValueError):
            DirectRenderer(device, tris, mats, 4, 4, **kw)
        with pytest.raises(ValueError):
            IndirectRenderer(device, tris, mats, 4, 4, **kw)
    r = IndirectRenderer(device, tris, mats, 4, 4, light_choice="power", candidates=1)   # 1: exactly the parent's calls
    u = IndirectRenderer(device, tris, mats, 4, 4)
    try:
        assert r._ris is None and r.candidates == 1
        with pytest.raises(ValueError):
            r.set_candidates(33)
        for bad in (dict(candidates=2), dict(candidates=1, through_ris=True)):
            with pytest.raises(ValueError):
                u.set_candidates(**bad)
    finally:
        r.release()
        u.release()


def test_set_candidates_between_renders(device):
    """one renderer, M changed between renders: 1 through the RIS entry point is the parent's image, 8 the restatement's"""
    name, W, H, frames, K, M, B, R, cap, mis = rc.PYTHON[1]
    tris, mats, lights, cam = ris_scene(name)
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, mis=mis, roulette=Roulette(R, cap), light_choice="power",
                         stripe_rows=1)
    try:
        with options(device, ACCEL=1):
            r.render(frames, 0)
            parent = r.read()
            r.set_candidates(1, through_ris=True)
            assert r._ris is not None
            r.render(frames, 0)
            assert_fb_equal(r.read(), parent, "M = 1 through the RIS entry point")
            r.set_candidates(M)
            r.render(frames, 0)
            assert_fb_equal(r.read(), rc.wanted(rc.PYTHON[1])[0], "M = %d after set_candidates" % M)
            r.set_candidates(1)
            assert r._ris is None
            r.render(frames, 0)
            assert_fb_equal(r.read(), parent, "back to the parent's calls")
    finally:
        r.release()


def test_adaptive_render_with_eight_candidates(device):
    """render_adaptive with candidates = 8 goes through pt_render_indirect_pixels_ris: each pixel holds the bits of the uniform RIS
    render after as many frames as it received"""
    name, W, H, _, K, M, B, R, cap, mis = rc.ADAPTIVE
    tris, mats, lights, cam = ris_scene(name)
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=K, max_bounces=B, mis=mis, roulette=Roulette(R, cap), moments=True,
                         light_choice="power", candidates=M, stripe_rows=1, chunk_frames=2)
    try:
        got = r.render_adaptive(0.3, min_samples=4, max_samples=12, frames_per_pass=2)
        fb, counts = r.read(), r.sample_counts()
    finally:
        r.release()
    assert np.array_equal(counts, got.counts) and len(got.passes) >= 2 and 0 < got.passes[-1] < got.passes[0] <= W * H, got.passes
    assert len(np.unique(counts)) >= 2, "every pixel stopped at the same count: nothing adaptive happened"
    for n in np.unique(counts):
        want = rs.render(tris, mats, W, H, 0, int(n), K, M, B=B, R=R, cap=cap, mis=mis, lights=lights, cam=cam)
        at = counts == n
        assert_fb_equal(fb[at], want[at], "the pixels that received %d frames" % n)


def test_cpp_harness_candidates(tmp_path):
    from gpu_support import harness_ppm
    from oclpathtracer_amd import scene

    tris, mats = scene.load_model()
    dim, frames = 24, 3
    out, name, pixels = harness_ppm(tmp_path, dim, frames, "DirectIllumination", "--lights", "power", "--candidates", "8")
    assert name.endswith("_power_ris8.ppm"), name
    want = rs.render(tris, mats, dim, dim, 0, frames, 4, 8)
    assert np.array_equal(pixels, scene.f2c(want[:, :3]))


def test_cpp_harness_candidates_indirect(tmp_path):
    """IndirectIllumination --candidates without --roulette: pt_render_indirect_ris with a first bounce no path reaches"""
    from gpu_support import harness_ppm
    from oclpathtracer_amd import scene

    tris, mats = scene.load_model()
    dim, frames = 24, 3
    out, name, pixels = harness_ppm(tmp_path, dim, frames, "IndirectIllumination", "--mis", "--lights", "power", "--candidates", "8")
    assert name.endswith("_mis_power_ris8.ppm"), name
    assert "(8 candidates per light sample)" in out
    want = rs.render(tris, mats, dim, dim, 0, frames, 1, 8, B=16, mis=True)
    assert np.array_equal(pixels, scene.f2c(want[:, :3]))


def test_cpp_harness_candidates_adaptive(tmp_path):
    """... with --roulette and --adaptive: the list passes go through pt_render_indirect_pixels_ris, two frames per pass from the fourth
    on, so every pixel shows the uniform RIS render of 4, 6, .. 12 frames, and the reported samples lie between what the matches allow"""
    from gpu_support import harness_ppm
    from oclpathtracer_amd import scene

    tris, mats = scene.load_model()
    dim = 24
    out, name, pixels = harness_ppm(tmp_path, dim, 2, "IndirectIllumination", "--mis", "--lights", "power", "--candidates", "8", "--roulette", "3,0.5",
                                    "--adaptive", "0.3,4,12")
    assert name.endswith("_mis_power_rr_ris8_adaptive.ppm"), name
    line = [l for l in out.splitlines() if l.startswith("adaptive:")][0]
    passes = [int(n) for n in line[line.index("[") + 1: line.index("]")].split()]
    samples = int(line.split()[-1])
    assert len(passes) >= 2 and 0 < passes[-1] <= passes[0] <= dim * dim, line
    assert samples == 4 * dim * dim + 2 * sum(passes), line
    counts = list(range(4, 14, 2))
    shown = np.stack([scene.f2c(rs.render(tris, mats, dim, dim, 0, n, 1, 8, B=16, R=3, cap=0.5, mis=True)[:, :3]) for n in counts])
    match = np.all(shown == pixels[None], axis=2)                     # [count, pixel]
    assert np.all(match.any(axis=0)), "%d pixels show no uniform RIS render of 4 .. 12 frames" % int((~match.any(axis=0)).sum())
    n = np.array(counts)[:, None]
    low, high = np.where(match, n, 99).min(axis=0).sum(), np.where(match, n, 0).max(axis=0).sum()
    assert low <= samples <= high, (low, samples, high)
    assert not np.all(match[0]) and not np.all(match[-1]), "every pixel stopped at the same count"
