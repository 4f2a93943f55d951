"""Light choice by power (pt_light_table, pt_render_direct_power, pt_render_indirect_power) on the MI355X, bit for bit.

The table -- cdf[0 .. nl] and tri_q -- is compared with tests/power_oracle.c for lists of every shape the build treats differently.
Every render of tests/power_cases.py -- at most 40 x 24 x 3 frames per call -- is compared twice with the restatement, NaN masks equal:
the sample workspace with the radiance before the fold, and the framebuffer.  tests/test_power_cpu.py proves, on these very inputs, that
q = 1 entries, the first and the last entry and an entry behind a q = 0 one are chosen, that the empty table is met and that the MIS
estimator's later hits read tri_q at counts of 1 and 2.  The identities need no restatement.  Lists of more than 70 020 entries, totals
from 2^32 on and the numeric domain of the powers are tests/test_gpu_light_scale.py's."""
import numpy as np
import pytest

import power_cases as pc
import power_oracle as po
import power_scenes as ps
from conftest import assert_fb_equal
from gpu_support import SEARCHES, assert_lit_argument_errors, harness_ppm, lit_with_samples, options, render
from indirect_edges import clamped_raw
from oclpathtracer_amd import scene, shim
from power_support import PowerBuffers, assert_table as _assert_table, power_with_samples
from scenes import edge_scene

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int32)
W, H, FRAMES = pc.W, pc.H, pc.FRAMES
MODES = pytest.mark.parametrize("mode", pc.MODES, ids=[pc.MODE_NAMES[m] for m in pc.MODES])
BLOCK, TILE = 256, 2048   # csrc/pt_kernels.h: PT_LIGHT_SCAN_BLOCK, PT_LIGHT_SCAN_TILE


# ---- the table -------------------------------------------------------------------------------------------------------------------
def test_table_of_the_scenes_lists(device, cornell):
    tris, mats = cornell
    _assert_table(device, tris, mats, scene.emitters(tris, mats), "the Cornell emitters")
    _assert_table(device, tris, mats, [11], "nl = 1")
    _assert_table(device, tris, mats, clamped_raw(len(tris)), "indices out of range")
    _assert_table(device, tris, mats, NONE, "nl = 0")
    ut, um = ps.unequal_lights()
    _assert_table(device, ut, um, scene.emitters(ut, um), "the unequal lights")
    _assert_table(device, ut, um, ps.edge_list(), "duplicates, unsorted, non-emitters")
    _assert_table(device, ut, um, ps.zero_list(), "the all-zero list")


@pytest.mark.parametrize("nl", [BLOCK - 1, BLOCK, BLOCK + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_table_sizes_about_the_scans_block_and_tile(device, nl):
    ut, um = ps.unequal_lights()
    rng = np.random.default_rng(nl)
    _assert_table(device, ut, um, rng.choice(ps.edge_list(), nl).astype(np.int32), "nl = %d" % nl)


def test_table_of_seventy_thousand_entries(device):
    tris, mats, _, _ = edge_scene("nested:15")[1]
    li = np.tile(scene.emitters(tris, mats), 2334).astype(np.int32)   # 30 x 2334 = 70 020 entries, 35 tiles
    assert len(tris) == 540 and 70000 <= len(li) < 71000
    _assert_table(device, tris, mats, li, "70 020 entries")


def test_table_rebuilt_into_the_same_buffers(device):
    from oclpathtracer_amd import adl

    ut, um = ps.unequal_lights()
    long_list, short_list = np.tile(ps.edge_list(), 12).astype(np.int32), scene.emitters(ut, um)[::-1].astype(np.int32)
    tables = (adl.Buffer(device, shim.load().pt_light_table_bytes(len(long_list)) // 8, np.uint64), adl.Buffer(device, len(ut), np.uint32))
    try:
        for li in (long_list, short_list, ps.zero_list()):
            _assert_table(device, ut, um, li, "%d entries into the same buffers" % len(li), tables=tables)
    finally:
        for b in tables:
            b.release()


def test_table_argument_errors(device, cornell):
    from oclpathtracer_amd import adl

    tris, mats = cornell
    lib, ntri, nmat = shim.load(), len(tris), len(mats)
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    assert lib.pt_light_table_bytes(-1) == 0 and lib.pt_light_table_bytes(1 << 24) == 0
    assert lib.pt_light_table_bytes(0) >= 8 and lib.pt_light_table_bytes(70020) >= 8 * 70021
    words = lib.pt_light_table_bytes(2) // 8
    tb, mb = adl.Buffer(device, ntri, scene.TRIANGLE_DTYPE), adl.Buffer(device, nmat, scene.MATERIAL_DTYPE)
    lb, qb, tq = adl.Buffer(device, 2, np.int32), adl.Buffer(device, words, np.uint64), adl.Buffer(device, ntri, np.uint32)
    small_q, small_t = adl.Buffer(device, words - 1, np.uint64), adl.Buffer(device, ntri - 1, np.uint32)
    big = adl.Buffer(device, 8 * words + 4 * ntri + 64, np.uint8)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    oq = adl.Buffer(other, words, np.uint64)
    try:
        tb.write(tris, ntri)
        mb.write(mats, nmat)
        lb.write(np.array([10, 11], np.int32), 2)
        sentinel = np.full(words, 0x0123456789abcdef, np.uint64)
        qb.write(sentinel, words)

        def call(t=tb, nt=ntri, m=mb, nm=nmat, l=lb, nl=2, q=qb, r=tq):
            t, m, l, q, r = (x._h if x is not None else None for x in (t, m, l, q, r))
            return lib.pt_light_table(device._h, t, nt, m, nm, l, nl, q, r, None)

        def wrap(off, nbytes):
            w = adl.Buffer()
            w.setRawPtr(device, big.m_ptr + off, nbytes)
            return w
        q0, q_odd, t_in, t_odd = wrap(0, 8 * words), wrap(4, 8 * words), wrap(8 * words - 4, 4 * ntri), wrap(8 * words + 2, 4 * ntri)
        try:
            for kw, code in [(dict(q=None), E_INV), (dict(r=None), E_INV), (dict(t=None), E_INV), (dict(m=None), E_INV), (dict(l=None), E_INV),
                             (dict(nl=-1), E_INV), (dict(nt=-1), E_INV), (dict(nm=0), E_INV), (dict(nl=1 << 24), E_INV),
                             (dict(nl=3), E_RANGE), (dict(nt=ntri + 1), E_RANGE), (dict(nm=nmat + 1), E_RANGE),
                             (dict(q=small_q), E_RANGE), (dict(r=small_t), E_RANGE), (dict(q=oq), E_INV),
                             (dict(q=q_odd), E_INV), (dict(q=q0, r=t_odd), E_INV), (dict(q=q0, r=t_in), E_INV), (dict(r=lb), E_RANGE)]:
                assert call(**kw) == code, kw
            assert call(q=tb) == E_INV                                       # the table over an input
        finally:
            for w in (q0, q_odd, t_in, t_odd):
                w.release()
        got = np.zeros(words, np.uint64)
        qb.read(got, words)
        device.waitForCompletion()
        assert np.array_equal(got, sentinel), "an error touched the table"
    finally:
        for b in (tb, mb, lb, qb, tq, small_q, small_t, big, oq):
            b.release()
        adl.DeviceUtils.deallocate(other)


# ---- renders against the restatement ---------------------------------------------------------------------------------------------
def _power(device, mode, name, lights, Ws, Hs, frames, K, B, **kw):
    tris, mats, cam = pc.scene_of(name)
    return power_with_samples(device, mode, (tris, mats, pc.lights_of(name, lights), cam), Ws, Hs, frames, K, B, **kw)


def _compare(device, mode, name, lights, Ws, Hs, frames, K, B, what, **stripes):
    what = "%s %s" % (pc.MODE_NAMES[mode], what)
    want_fb, want_rad = pc.wanted(mode, name, lights, Ws, Hs, frames, K, B, **stripes)
    fb, ws = _power(device, mode, name, lights, Ws, Hs, frames, K, B, **stripes)
    assert_fb_equal(ws[:frames], want_rad, what + ": radiance before the fold")
    assert_fb_equal(fb, want_fb, what)


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_every_search_on_the_cornell_box(device, quad, accel):
    K, B = pc.SEARCH_KB
    for mode in pc.MODES:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            _compare(device, mode, "cornell", None, W, H, FRAMES, K, B, "q%d a%d" % (quad, accel))


@MODES
def test_tiled_brute_force(device, mode):
    assert 257 <= len(pc.scene_of(pc.BIG[0])[0]) <= 511
    with options(device, ACCEL=1):
        _compare(device, mode, pc.BIG[0], None, W, H, FRAMES, *pc.BIG_KB, "tiled brute force, 20 unequal emitters")


@MODES
@pytest.mark.parametrize("accel", [0, 2, 1])
def test_lbvh_and_forced_brute_force(device, mode, accel):
    assert len(pc.scene_of(pc.BIG[1])[0]) >= 512
    with options(device, ACCEL=accel):
        _compare(device, mode, pc.BIG[1], None, W, H, FRAMES, *pc.BIG_KB, "540 triangles, 30 unequal emitters, accel %d" % accel)


@MODES
@pytest.mark.parametrize("lights", [None, "edges", "zero"], ids=["emitters", "edges", "zero"])
def test_unequal_lights(device, mode, lights):
    """the room of one panel and dozens of dim emitters: its own list, the list made for the choice's edges, and the empty table"""
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            _compare(device, mode, "unequal", lights, W, H, FRAMES, *pc.EDGE_KB, "unequal lights, list %s, accel %d" % (lights, accel))


@MODES
def test_indices_out_of_range_are_clamped(device, cornell, mode):
    """[-1, 10, ntri + 5, 11] through the C ABI, the table and the counts made from that same list: the image of [0, 10, 35, 11]"""
    tris, mats = cornell
    K, B = pc.SEARCH_KB
    raw = clamped_raw(len(tris))
    want_fb, want_rad = pc.wanted(mode, "cornell", "clamped", W, H, FRAMES, K, B)
    b = PowerBuffers(mode, device, tris, mats, W, H, lights=raw, frames=FRAMES, pad=0)
    try:
        kw = {} if mode == po.DIRECT else dict(max_bounces=B)
        assert b.call(b.params(len(raw), frame_count=FRAMES, light_samples=K, **kw)) == shim.PT_OK
        assert_fb_equal(b.read(), want_fb, "clamped list")
        assert_fb_equal(b.read(b.sb, np.zeros((FRAMES * W * H, 3), np.float32)), want_rad.reshape(-1, 3), "clamped list: radiance before the fold")
    finally:
        b.release()


@MODES
def test_small_images(device, mode):
    """1, 15 and 65 pixels: one sample; one partial wave; a full wave and one lane"""
    for Ws, Hs, B in pc.SMALL:
        for name, accel in (("unequal", 1), ("nested:15", 2)):
            with options(device, ACCEL=accel):
                _compare(device, mode, name, None, Ws, Hs, 2, 4, B, "%s %dx%d accel %d" % (name, Ws, Hs, accel))


@MODES
def test_three_rank_stripes(device, mode):
    for r in range(pc.RANKS):
        _compare(device, mode, "unequal", None, W, H, 2, 1, 4, "rank %d of %d" % (r, pc.RANKS), stripe_rows=pc.STRIPE_ROWS, n_ranks=pc.RANKS, rank=r)


@MODES
def test_a_chunked_workspace(device, mode):
    want = pc.wanted(mode, "unequal", None, W, H, FRAMES, 1, 4)[0]
    assert_fb_equal(_power(device, mode, "unequal", None, W, H, FRAMES, 1, 4, chunk_frames=1)[0], want, "a workspace of one frame: three launches, three folds")


@MODES
@pytest.mark.parametrize("K,B", pc.PARAM_KB)
def test_light_samples_and_bounces(device, mode, K, B):
    _compare(device, mode, "unequal", None, 24, 16, 2, K, B, "K%d B%d" % (K, B))


# ---- identities ------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("lights", [(10,), (11, 11), (10, 10, 10, 10)], ids=["nl1", "nl2", "nl4"])
def test_equal_powers_reproduce_the_uniform_parent(device, cornell, mode, lights):
    """duplicates of one emitter: inv is exactly nl and the entry exactly floor(u nl / 2^24) -- the parent's workspace and image"""
    tris, mats = cornell
    B = None if mode == po.DIRECT else 4
    sc = (tris, mats, np.asarray(lights, np.int32), None)
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            want_fb, want_ws = lit_with_samples(device, sc, W, H, FRAMES, 2, max_bounces=B, mis=mode == po.MIS)
            fb, ws = power_with_samples(device, mode, sc, W, H, FRAMES, 2, B)
            assert_fb_equal(ws, want_ws, "nl %d accel %d: radiance before the fold" % (len(lights), accel))
            assert_fb_equal(fb, want_fb, "nl %d accel %d" % (len(lights), accel))


@MODES
def test_no_lights_and_a_null_table_is_the_renderer(device, cornell, mode):
    tris, mats = cornell
    B = 1 if mode == po.DIRECT else 3
    want = render(device, tris, mats, W, H, FRAMES, depth=B, stripe_rows=1)
    b = PowerBuffers(mode, device, tris, mats, W, H, frames=FRAMES, pad=0)
    try:
        kw = {} if mode == po.DIRECT else dict(max_bounces=B)
        assert b.call(b.params(0, frame_count=FRAMES, light_samples=4, **kw), lb=None, cb=None, qb=None, tq=None) == shim.PT_OK
        assert_fb_equal(b.read(), want, "no lights, NULL table against Renderer.render(max_bounces=%d)" % B)
    finally:
        b.release()
    assert_fb_equal(power_with_samples(device, mode, (tris, mats, NONE, None), W, H, FRAMES, 4, B)[0], want, "lights=[] through the renderer")


@pytest.mark.parametrize("mis", [False, True])
def test_one_bounce_is_direct_illumination_by_power(device, mis):
    want = _power(device, po.DIRECT, "unequal", "edges", W, H, FRAMES, 4, 1)[0]
    assert_fb_equal(_power(device, po.MIS if mis else po.INDIRECT, "unequal", "edges", W, H, FRAMES, 4, 1)[0], want, "B = 1 against direct")


def test_a_uniform_renderer_beside_a_power_one_is_unmoved(device):
    """both over one Renderer's buffers, renders interleaved: each is still its own restatement's"""
    import mis_oracle as mo
    from oclpathtracer_amd.render import Renderer

    tris, mats = ps.unequal_lights()
    K, B = 1, 4
    r = Renderer(device, tris, mats, W, H, stripe_rows=1)
    uniform = r.indirect_renderer(light_samples=K, max_bounces=B, chunk_frames=FRAMES, mis=True)
    power = r.indirect_renderer(light_samples=K, max_bounces=B, chunk_frames=FRAMES, mis=True, light_choice="power")
    direct = r.direct_renderer(light_samples=K, chunk_frames=FRAMES, light_choice="power")
    try:
        assert uniform.light_choice == "uniform" and uniform.cdf is None and power.cdf is not None and direct.tri_q is not None
        power.render(2)
        uniform.render(FRAMES)
        direct.render(FRAMES)
        power.render(1)
        assert_fb_equal(uniform.read(), mo.render(tris, mats, W, H, 0, FRAMES, K, B), "uniform beside power")
        assert_fb_equal(power.read(), pc.wanted(po.MIS, "unequal", None, W, H, FRAMES, K, B)[0], "power beside uniform")
        assert_fb_equal(direct.read(), pc.wanted(po.DIRECT, "unequal", None, W, H, FRAMES, K, 1)[0], "direct by power on the same buffers")
    finally:
        for x in (direct, power, uniform):
            x.release()
        r.release()
    assert power.cdf is None and power.counts is None
    with pytest.raises(ValueError):
        Renderer(device, tris, mats, W, H).direct_renderer(light_choice="brightest")


# ---- errors ----------------------------------------------------------------------------------------------------------------------
@MODES
def test_argument_errors_leave_the_framebuffer_untouched(device, cornell, mode):
    from oclpathtracer_amd import adl

    tris, mats = cornell
    Ws, Hs, ntri = 16, 8, len(tris)
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    b = PowerBuffers(mode, device, tris, mats, Ws, Hs)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    oq = adl.Buffer(other, 8, np.uint64)
    short_q, short_t = adl.Buffer(device, 2, np.uint64), adl.Buffer(device, ntri - 1, np.uint32)
    big = adl.Buffer(device, 12 * Ws * Hs + 4 * ntri + 64, np.uint8)
    try:
        p = b.params(2)
        assert b.call(p, qb=None) == E_INV and b.call(p, tq=None) == E_INV     # NULL with nl > 0
        assert b.call(p, qb=short_q) == E_RANGE and b.call(p, tq=short_t) == E_RANGE   # 8 x (nl + 1) bytes, one triangle short
        assert b.call(p, qb=oq) == E_INV                                      # of another device

        def wrap(off, nbytes):
            w = adl.Buffer()
            w.setRawPtr(device, big.m_ptr + off, nbytes)
            return w
        s0, q_in, q_odd, t_odd = wrap(0, 12 * Ws * Hs), wrap(12 * Ws * Hs - 8, 24), wrap(12 * Ws * Hs + 4, 24), wrap(12 * Ws * Hs + 2, 4 * ntri)
        q_ok, t_in = wrap(12 * Ws * Hs, 24), wrap(12 * Ws * Hs + 16, 4 * ntri)
        try:
            assert b.call(p, sb=s0, qb=q_in) == E_INV                         # cdf overlapping the workspace
            assert b.call(p, sb=s0, qb=q_odd) == E_INV                        # cdf not 8-byte aligned
            assert b.call(p, sb=s0, tq=t_odd) == E_INV                        # tri_q not 4-byte aligned
            assert b.call(p, sb=s0, qb=q_ok, tq=t_in) == E_INV                # cdf and tri_q overlapping
        finally:
            for w in (s0, q_in, q_odd, t_odd, q_ok, t_in):
                w.release()
        if mode != po.DIRECT:
            assert b.call(p, mis=2) == E_INV
            for kw in [dict(max_bounces=0), dict(max_bounces=65536)] + [dict(reserved=k) for k in range(4)]:
                assert b.call(b.params(2, **kw)) == E_INV, kw
            if mode == po.MIS:
                assert b.call(p, cb=None) == E_INV                            # mis = 1 needs the counts
            else:
                assert b.call(p, cb=None) == shim.PT_OK                       # mis = 0: the counts may be NULL
                b.fb.write(b.sentinel, len(b.sentinel))
        else:
            for k in range(5):
                assert b.call(b.params(2, reserved=k)) == E_INV, k
        assert_lit_argument_errors(b)                                         # what every entry point rejects, the framebuffer untouched
    finally:
        b.release()
        for x in (oq, short_q, short_t, big):
            x.release()
        adl.DeviceUtils.deallocate(other)


# ---- the C++ harness -------------------------------------------------------------------------------------------------------------
def test_cpp_harness_direct_by_power(tmp_path, cornell):
    tris, mats = cornell
    out, name, pixels = harness_ppm(tmp_path, 32, 3, "DirectIllumination", "--lights", "power")
    assert "DirectIllumination (lights by power):" in out and name.startswith("directIllumination_") and name.endswith("_power.ppm")
    assert np.array_equal(pixels, scene.f2c(po.render(po.DIRECT, tris, mats, 32, 32, 0, 3, 4)[:, :3]))


@pytest.mark.parametrize("mis", [False, True])
def test_cpp_harness_indirect_by_power(tmp_path, cornell, mis):
    tris, mats = cornell
    out, name, pixels = harness_ppm(tmp_path, 32, 3, "IndirectIllumination", "--lights", "power", *(["--mis"] if mis else []))
    assert "(lights by power):" in out and name.endswith("_mis_power.ppm" if mis else "_power.ppm")
    assert np.array_equal(pixels, scene.f2c(po.render(po.MIS if mis else po.INDIRECT, tris, mats, 32, 32, 0, 3, 1, 16)[:, :3]))
