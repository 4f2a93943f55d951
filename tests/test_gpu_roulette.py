"""Russian roulette (pt_render_indirect_rr) on the MI355X, bit for bit.

Every render is compared twice with the restatement (tests/roulette_oracle.c), NaN positions equal: the sample workspace with the
radiance before the fold, and the framebuffer.  The inputs are tests/roulette_cases.py's -- at most 24 x 16 x 3 frames per call, or a
few hundred samples about a wave and about a run of the refilling kernel --; tests/test_roulette_cpu.py proves on these very inputs
that every edge of the roulette is reached.  The identities (first_bounce >= max_bounces is the parent's image; no lights is the
renderer's) need no restatement.  r == q exactly is met by no input (tests/test_roulette_cpu.py counts), so nothing is asserted of it."""
import ctypes

import numpy as np
import pytest

import direct_oracle as do
import roulette_cases as rc
import roulette_oracle as ro
from conftest import assert_fb_equal
from gpu_support import SEARCHES, assert_lit_argument_errors, lit_with_samples, options, render
from oclpathtracer_amd import shim
from oclpathtracer_amd.camera import Camera
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette
from power_support import power_with_samples
from roulette_support import RouletteBuffers, roulette_with_samples
from scenes import edge_scene
import power_oracle as po

pytestmark = pytest.mark.gpu

EST = pytest.mark.parametrize("mis,power", rc.ESTIMATORS, ids=rc.EST_IDS)
NONE = np.zeros(0, np.int32)


def _compare(device, case, what, **kw):
    name, Ws, Hs, frames, K, B, R, cap, mis, power = case
    what = "%s %s K%d B%d R%d cap %g mis %d power %d" % (what, name, K, B, R, cap, mis, power)
    want_fb, want_rad = rc.wanted(*case, **kw)
    fb, ws = roulette_with_samples(device, edge_scene(name)[1], Ws, Hs, frames, K, B, R, cap, mis=mis, power=power, **kw)
    assert_fb_equal(ws[:frames], want_rad, what + ": radiance before the fold")
    assert_fb_equal(fb, want_fb, what)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_parity_on_the_cornell_box_under_every_search(device, quad, accel):
    """R in {1, 3} x cap in {1, 0.95, 0.25} x the four estimators x K in {1, 2}, B = 16"""
    rc.prefetch(rc.parity_cases())
    with options(device, QUAD_FILTER=quad, ACCEL=accel):
        for case in rc.parity_cases():
            _compare(device, case, "q%d a%d" % (quad, accel))


@pytest.mark.parametrize("accel", [1, 2])
def test_parity_in_a_glossy_finite_room(device, accel):
    rc.prefetch(rc.big_cases(rc.GLOSSY))
    with options(device, ACCEL=accel):
        for case in rc.big_cases(rc.GLOSSY):
            _compare(device, case, "accel %d" % accel)


@pytest.mark.parametrize("accel", [0, 2, 1])
def test_parity_on_a_scene_that_takes_the_lbvh_by_itself(device, accel):
    assert len(edge_scene(rc.LBVH[0])[1][0]) >= 512
    rc.prefetch(rc.big_cases(rc.LBVH))
    with options(device, ACCEL=accel):
        for case in rc.big_cases(rc.LBVH):
            _compare(device, case, "accel %d" % accel)


def test_parity_on_the_tiled_brute_force_table(device):
    assert 257 <= len(edge_scene(rc.TILED[0])[1][0]) <= 511
    rc.prefetch(rc.big_cases(rc.TILED))
    with options(device, ACCEL=1):
        for case in rc.big_cases(rc.TILED):
            _compare(device, case, "tiled")


# ---- 2. identity ---------------------------------------------------------------------------------------------------------------
@EST
@pytest.mark.parametrize("R", ["B", ro.NEVER])
def test_no_roulette_is_the_parent_entry_point(device, mis, power, R):
    """first_bounce >= max_bounces: the parent's workspace and framebuffer, by the refilling kernel (accel 1) and by the LBVH (accel 2)"""
    K, B = 2, 5
    R = B if R == "B" else R
    for name in ("cornell", "finite:5"):
        sc = edge_scene(name)[1]
        for accel in (1, 2):
            with options(device, ACCEL=accel):
                if power:
                    want_fb, want_ws = power_with_samples(device, po.MIS if mis else po.INDIRECT, sc, rc.W, rc.H, rc.FRAMES, K, B)
                else:
                    want_fb, want_ws = lit_with_samples(device, sc, rc.W, rc.H, rc.FRAMES, K, max_bounces=B, mis=mis)
                fb, ws = roulette_with_samples(device, sc, rc.W, rc.H, rc.FRAMES, K, B, R, 0.25, mis=mis, power=power)
                assert_fb_equal(ws, want_ws, "%s accel %d: radiance before the fold" % (name, accel))
                assert_fb_equal(fb, want_fb, "%s accel %d" % (name, accel))


@EST
def test_no_lights_and_no_roulette_is_the_renderer(device, cornell, mis, power):
    tris, mats = cornell
    B = 4
    want = render(device, tris, mats, rc.W, rc.H, rc.FRAMES, depth=B, stripe_rows=1)
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            fb = roulette_with_samples(device, (tris, mats, NONE, None), rc.W, rc.H, rc.FRAMES, 2, B, B, 0.5, mis=mis, power=power)[0]
            assert_fb_equal(fb, want, "no lights, R = B, accel %d against Renderer.render(max_bounces=%d)" % (accel, B))
    b = RouletteBuffers(device, tris, mats, rc.W, rc.H, mis=mis, power=power, frames=rc.FRAMES, pad=0)
    try:   # through the C ABI: every optional handle NULL
        p = b.params(0, frame_count=rc.FRAMES, light_samples=4, max_bounces=B)
        assert b.call(p, rr=b.roulette(ro.NEVER, 1.0), lb=None, cb=None, qb=None, tq=None) == shim.PT_OK
        assert_fb_equal(b.read(), want, "no lights, NULL handles")
    finally:
        b.release()


# ---- 3. refill edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.refill_counts(), ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("B", [1, 2, 8])
def test_refill_about_a_wave_and_about_a_run(device, n, B):
    """n items in one launch of the brute-force kernel, R = 1 and cap = 0.25: lanes die at different vertices and take new items mid-run;
    B = 1: no roulette, every lane refills in every iteration"""
    Ws, Hs, frames = rc.refill_shape(n)
    assert Ws * Hs * frames == n
    with options(device, ACCEL=1):
        for mis, power in rc.ESTIMATORS if B == 8 else rc.ESTIMATORS[:2]:
            _compare(device, ("cornell", Ws, Hs, frames, 1, B, 1, 0.25, mis, power), "%d items" % n)


def test_refill_on_the_tiled_table_and_on_the_lbvh(device):
    n = 3 * rc.rr_run() + 7
    Ws, Hs, frames = rc.refill_shape(n)
    for name, accel in ((rc.TILED[0], 1), (rc.LBVH[0], 2)):
        with options(device, ACCEL=accel):
            _compare(device, (name, Ws, Hs, frames, 1, 8, 1, 0.25, True, False), "%d items accel %d" % (n, accel))


# ---- 4. the roulette's edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", sorted(rc.EDGES))
def test_roulette_edges(device, edge):
    name, Ws, Hs, frames, K, B, R, cap, mis = rc.EDGES[edge]
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            _compare(device, (name, Ws, Hs, frames, K, B, R, cap, mis, False), "%s accel %d" % (edge, accel))


# ---- 5. layout -----------------------------------------------------------------------------------------------------------------
LAYOUT = ("cornell", rc.W, rc.H, 5, 1, 8, 1, 0.5, True, False)


@pytest.mark.parametrize("accel", [1, 2])
def test_a_workspace_of_two_frames_for_five(device, accel):
    with options(device, ACCEL=accel):
        fb = roulette_with_samples(device, edge_scene("cornell")[1], rc.W, rc.H, 5, 1, 8, 1, 0.5, mis=True, chunk_frames=2)[0]
    assert_fb_equal(fb, rc.wanted(*LAYOUT)[0], "three chunks: 2 + 2 + 1 frames")


@pytest.mark.parametrize("accel", [1, 2])
def test_resuming_a_mean(device, accel):
    tris, mats, lights, cam = edge_scene("cornell")[1]
    with options(device, ACCEL=accel):
        r = IndirectRenderer(device, tris, mats, rc.W, rc.H, light_samples=1, max_bounces=8, mis=True, roulette=Roulette(1, 0.5), stripe_rows=1,
                             chunk_frames=3)
        try:
            r.render(2)
            r.render(3)
            assert r.frames_done == 5
            assert_fb_equal(r.read(), rc.wanted(*LAYOUT)[0], "frames [0, 2) then [2, 5)")
            ws = np.zeros((3, r.local_pixels, 3), np.float32)
            r.samples.read(ws, ws.size)
            device.waitForCompletion()
            gid, frame = do.sample_ids(rc.W, rc.H, 3)
            want = ro.samples(tris, mats, rc.W, rc.H, gid, frame + 2, 1, 8, 1, 0.5, mis=True)[0].reshape(3, -1, 3)
            assert_fb_equal(ws, want, "the workspace of frames [2, 5)")
        finally:
            r.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_three_rank_stripes_assemble_to_the_one_device_image(device, accel):
    name, Ws, Hs, frames, K, B, R, cap, mis, power = case = ("cornell", 24, 19, 2, 1, 6, 1, 0.5, True, True)
    whole = np.zeros((Ws * Hs, 4), np.float32)
    with options(device, ACCEL=accel):
        for rank in range(3):
            st = dict(stripe_rows=3, n_ranks=3, rank=rank)
            _compare(device, case, "rank %d of 3" % rank, **st)
            whole[do.local_gids(Ws, Hs, **st)] = roulette_with_samples(device, edge_scene(name)[1], Ws, Hs, frames, K, B, R, cap, mis=mis, power=power, **st)[0]
        one = roulette_with_samples(device, edge_scene(name)[1], Ws, Hs, frames, K, B, R, cap, mis=mis, power=power)[0]
    assert_fb_equal(whole, one, "the stripes of three ranks against one device")
    assert_fb_equal(one, rc.wanted(*case)[0], "one device")


@pytest.mark.parametrize("accel", [1, 2])
def test_a_camera_of_ones_own(device, accel):
    tris, mats, _, _ = edge_scene("cornell")[1]
    cam = Camera(eye=(-2.0, 1.0, 3.0), center=(1.0, 3.0, -2.0), up=(0.1, 1.0, 0.0), fov_y_deg=75.0)
    gid, frame = do.sample_ids(rc.W, rc.H, 2)
    with options(device, ACCEL=accel):
        fb, ws = roulette_with_samples(device, (tris, mats, None, cam), rc.W, rc.H, 2, 2, 6, 2, 0.5, mis=True)
    assert_fb_equal(ws, ro.samples(tris, mats, rc.W, rc.H, gid, frame, 2, 6, 2, 0.5, mis=True, cam=cam)[0].reshape(2, -1, 3), "camera: radiance")
    assert_fb_equal(fb, ro.render(tris, mats, rc.W, rc.H, 0, 2, 2, 6, 2, 0.5, mis=True, cam=cam), "camera")


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
@EST
def test_argument_errors_leave_the_framebuffer_untouched(device, cornell, mis, power):
    tris, mats = cornell
    E_INV = shim.PT_ERR_INVALID
    b = RouletteBuffers(device, tris, mats, 16, 8, mis=mis, power=power)
    try:
        p = b.params(2)
        assert b.call(p, rr=None) == E_INV                                              # a NULL pt_roulette
        for fb_ in (0, -1, -(1 << 31)):
            assert b.call(p, rr=b.roulette(first_bounce=fb_)) == E_INV, fb_              # first_bounce < 1
        for cap in (float("nan"), 0.0, -0.0, -0.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), float("inf"), -float("inf")):
            assert b.call(p, rr=b.roulette(max_survival=cap)) == E_INV, cap              # NaN or outside (0, 1]
        for k in range(2):
            assert b.call(p, rr=b.roulette(reserved=k)) == E_INV, k                      # a reserved word not 0
        assert b.call(p, qb=b.qb, tq=None) == E_INV and b.call(p, qb=None, tq=b.tq) == E_INV   # exactly one of cdf / tri_q, nl > 0
        assert b.call(p, mis=2) == E_INV
        for kw in [dict(max_bounces=0), dict(max_bounces=65536)] + [dict(reserved=k) for k in range(4)]:
            assert b.call(b.params(2, **kw)) == E_INV, kw
        if mis:
            assert b.call(p, cb=None) == E_INV                                          # mis = 1 needs the counts
        b.assert_untouched()
        assert b.call(p, rr=b.roulette(1, float(np.nextafter(np.float32(0.0), np.float32(1.0))))) == shim.PT_OK   # the smallest cap
        assert b.call(p, rr=b.roulette(0x7fffffff, 1.0)) == shim.PT_OK                                            # the largest R
        b.fb.write(b.sentinel, len(b.sentinel))
        assert_lit_argument_errors(b)                                                   # what every lit entry point rejects
    finally:
        b.release()


# ---- 7. Python -----------------------------------------------------------------------------------------------------------------
class _Recorder:
    """the library with the names of the render entry points that were called"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("pt_render_"):
            self.calls.append(name)
        return fn


@EST
def test_roulette_none_makes_exactly_todays_calls(device, cornell, mis, power):
    tris, mats = cornell
    parent = "pt_render_indirect_power" if power else "pt_render_indirect_mis" if mis else "pt_render_indirect"
    for roulette, entry in ((None, parent), (3, "pt_render_indirect_rr"), (Roulette(2, 0.5), "pt_render_indirect_rr")):
        r = IndirectRenderer(device, tris, mats, 16, 8, max_bounces=4, mis=mis, light_choice="power" if power else "uniform", roulette=roulette,
                             stripe_rows=1)
        try:
            r._lib = rec = _Recorder(r._lib)
            r.render(2)
            r.read()
            assert rec.calls == [entry], (roulette, rec.calls)
        finally:
            r._lib = rec._lib
            r.release()
    assert Roulette.of(3) == Roulette(3, 0.95) and Roulette.of(None) is None and Roulette() == (3, 0.95)
    for bad in (dict(first_bounce=0), dict(max_survival=0.0), dict(max_survival=1.5), dict(max_survival=float("nan")), dict(first_bounce=1.5)):
        with pytest.raises(ValueError):
            Roulette(**bad)
    with pytest.raises(TypeError):
        IndirectRenderer(device, tris, mats, 16, 8, roulette="often")


def test_renderer_options_compose(device, cornell):
    """Renderer.indirect_renderer(roulette=...) with mis, the choice by power and moments: the restatement's image, every frame counted"""
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    frames, K, B = 5, 1, 8
    base = Renderer(device, tris, mats, rc.W, rc.H, stripe_rows=1)
    r = base.indirect_renderer(light_samples=K, max_bounces=B, mis=True, light_choice="power", roulette=2, moments=True, chunk_frames=2)
    try:
        assert r.roulette == Roulette(2, 0.95)
        r.render(frames)
        want = ro.render(tris, mats, rc.W, rc.H, 0, frames, K, B, 2, 0.95, mis=True, power=True)
        assert_fb_equal(r.read(), want, "roulette with mis, power and moments")
        noise = r.noise()
        assert noise.samples + noise.rejected == frames * rc.W * rc.H, noise
        var, n = r.variance()
        gid, frame = do.sample_ids(rc.W, rc.H, frames)
        rad = ro.samples(tris, mats, rc.W, rc.H, gid, frame, K, B, 2, 0.95, mis=True, power=True)[0].reshape(frames, -1, 3)
        assert np.array_equal(n, np.isfinite(rad).all(axis=2).sum(axis=0).astype(np.uint32)), "the moments' counts"
        assert r.render_until(0.0, frames + 2) == frames + 2
        assert_fb_equal(r.read(), ro.render(tris, mats, rc.W, rc.H, 0, frames + 2, K, B, 2, 0.95, mis=True, power=True), "render_until")
    finally:
        r.release()
        base.release()


def test_a_cut_short_search_is_reported(device):
    from gpu_support import assert_cut_short_search_is_reported

    tris, mats, _, _ = edge_scene(rc.LBVH[0])[1]
    assert_cut_short_search_is_reported(device, lambda: IndirectRenderer(device, tris, mats, 16, 16, max_bounces=4, mis=True, roulette=1))


# ---- the C++ harness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,suffix,mis,power", [((), "_rr.ppm", False, False), (("--mis", "--lights", "power"), "_mis_power_rr.ppm", True, True)],
                         ids=["plain", "mis_power"])
def test_cpp_harness_with_roulette(tmp_path, cornell, flags, suffix, mis, power):
    from gpu_support import harness_ppm
    from oclpathtracer_amd import scene

    tris, mats = cornell
    out, name, pixels = harness_ppm(tmp_path, 32, 3, "IndirectIllumination", "--roulette", "2,0.5", *flags)
    assert "(roulette from 2, at most 0.5)" in out and name.startswith("indirectIllumination_") and name.endswith(suffix), (out, name)
    assert np.array_equal(pixels, scene.f2c(ro.render(tris, mats, 32, 32, 0, 3, 1, 16, 2, 0.5, mis=mis, power=power)[:, :3]))


def test_cpp_harness_with_roulette_and_noise(tmp_path):
    from gpu_support import harness_ppm

    out, name, _ = harness_ppm(tmp_path, 32, 5, "IndirectIllumination", "--roulette", "3", "--mis", "--noise")
    assert "(roulette from 3, at most 0.95)" in out and name.endswith("_mis_rr.ppm")
    line = [l for l in out.splitlines() if l.startswith("noise:")][0].split()
    assert int(line[line.index("samples") + 1]) + int(line[line.index("rejected") + 1]) == 32 * 32 * 5, line
