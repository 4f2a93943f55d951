"""The masked closest-hit search of the trace kernel (csrc/pt_kernels.hip: pt_intersect_masked<true, 1> -- own steps, the pending-pair
list, the tail's rounds, the merge) on the device, where the renders of the other tests rarely take it: dense masks, many accepted
triangles per ray, ties, dead lanes that bring masks, the 24 / 25-lane boundary of the own steps.

  1. pt_search_check_kernel calls the library's search on the rays, masks and lanes of tests/masked_search_cases.py, one wave per
     case; every lane must return the reference's winner -- argmin (t, index) over the masked triangles its test accepts -- in
     index, t, u and v, bit for bit.  tests/test_masked_search_cpu.py proves the expectation against the CPU oracle.
  2. the launcher's argument errors.
  3. renders of scenes.sheets() and its alternating form against the CPU oracle, image and ray count, with the primary and the
     secondary masks both on and both off; with them on both tables stand and the primary masks are as dense as the oracle's
     accepted sets at least: the dense masks reached the kernel.
"""
import ctypes

import numpy as np
import pytest

import masked_search_cases as msc
import scenes
from conftest import assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import adl, scene as _scene, shim
from test_gpu_secondary_masks import no_table

pytestmark = pytest.mark.gpu


def _launch(device, bufs, ntri, cases):
    k = device.getKernel("PtShimTest", "SearchCheckKernel")
    assert k is not None
    launcher = adl.Launcher(device, k)
    launcher.setBuffers([adl.BufferInfo(b) for b in bufs])
    launcher.setConst(np.int32(ntri))
    launcher.setConst(np.uint32(cases))
    launcher.launch1D(1)


def _run(device, tris, rays, masks):
    """rays float32 [cases, 64, 8], masks uint32 [cases, 64, 2] -> uint32 [cases, 64, 8]: hidx, t, hu, hv, steps, 0, 0, 0"""
    cases = len(rays)
    assert rays.shape == (cases, 64, 8) and masks.shape == (cases, 64, 2)
    tbuf = adl.Buffer(device, len(tris), _scene.TRIANGLE_DTYPE)
    rbuf = adl.Buffer(device, cases * 512, np.float32)
    mbuf = adl.Buffer(device, cases * 128, np.uint32)
    obuf = adl.Buffer(device, cases * 512, np.uint32)
    try:
        tbuf.write(np.ascontiguousarray(tris), len(tris))
        rbuf.write(np.ascontiguousarray(rays, np.float32).reshape(-1), cases * 512)
        mbuf.write(np.ascontiguousarray(masks, np.uint32).reshape(-1), cases * 128)
        obuf.write(np.full(cases * 512, 0xDEADBEEF, np.uint32), cases * 512)
        _launch(device, [tbuf, rbuf, mbuf, obuf], len(tris), cases)
        res = np.empty(cases * 512, np.uint32)
        obuf.read(res, cases * 512)
        device.waitForCompletion()
    finally:
        for b in (tbuf, rbuf, mbuf, obuf):
            b.release()
    return res.reshape(cases, 64, 8)


@pytest.mark.parametrize("name", msc.NAMES)
def test_every_lane_returns_the_reference_winner(device, name):
    tris = msc.scene(name)[0]
    cs = msc.cases(name)
    rays, masks = msc.device_input(name)
    got = _run(device, tris, rays, masks)
    steps = got[:, :, 4]
    print("%s: %d waves, %.2f steps per search, %d at the most" % (name, len(cs), steps[:, 0].mean(), steps.max()))
    assert not got[:, :, 5:].any(), name + ": the words behind the step count are not zero"
    assert (steps == steps[:, :1]).all(), name + ": the step count is not wave-uniform"
    bad = []
    for c, g in zip(cs, got):
        if not np.array_equal(g[:, 0], c.want[:, 0]):
            lane = int(np.flatnonzero(g[:, 0] != c.want[:, 0])[0])
            bad.append("%s: lane %d returns triangle %d, the reference's winner is %d" % (c.name, lane, np.int32(g[lane, 0]), np.int32(c.want[lane, 0])))
            continue
        try:
            assert_fb_equal(g[:, 1:4].view(np.float32), c.want[:, 1:4].view(np.float32), c.name + " (t, u, v)")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "%d of %d waves differ:\n%s" % (len(bad), len(cs), "\n".join(bad[:12]))


def test_argument_errors(device):
    tris = msc.scene("cornell")[0]
    t = adl.Buffer(device, 36, _scene.TRIANGLE_DTYPE)
    r = adl.Buffer(device, 2 * 512, np.float32)
    m = adl.Buffer(device, 2 * 128, np.uint32)
    o = adl.Buffer(device, 2 * 512, np.uint32)
    nan = adl.Buffer(device, 36, _scene.TRIANGLE_DTYPE)
    huge = adl.Buffer(device, 36, _scene.TRIANGLE_DTYPE)
    try:
        t.write(np.ascontiguousarray(tris), 36)
        bad = tris.copy()
        bad["p2"][5, 1] = np.nan
        nan.write(np.ascontiguousarray(bad), 36)
        big = tris.copy()
        for f in ("p1", "p2", "p3"):
            big[f][:, :3] *= np.float32(1e10)      # (the scene's extent lifts the determinant's bound over PT_DET_BOUND_MAX)
        huge.write(np.ascontiguousarray(big), 36)
        r.write(np.zeros(2 * 512, np.float32), 2 * 512)
        m.write(np.zeros(2 * 128, np.uint32), 2 * 128)
        sentinel = np.full(2 * 512, 0xDEADBEEF, np.uint32)
        o.write(sentinel, 2 * 512)

        def refused(bufs, ntri, cases, what):
            with pytest.raises(shim.ShimError) as e:
                _launch(device, bufs, ntri, cases)
            assert e.value.code == shim.PT_ERR_ARGS, what

        refused([t, r, m, o], 0, 2, "no triangle")
        refused([t, r, m, o], 65, 2, "65 triangles")
        refused([t, r, m, o], -1, 2, "a negative count")
        refused([t, r, m, o], 37, 2, "more triangles than the buffer holds")
        refused([t, r, m, o], 36, 3, "more cases than the ray, mask and result buffers hold")
        refused([t, r, m, o], 36, 65537, "too many cases")
        refused([t, m, m, o], 36, 2, "a ray buffer too small")
        refused([t, r, m, m], 36, 2, "a result buffer too small")
        refused([t, r, m, r], 36, 2, "the results over the rays")
        refused([t, r, m], 36, 2, "three buffers")
        refused([nan, r, m, o], 36, 2, "a scene with a NaN")
        refused([huge, r, m, o], 36, 2, "a scene that is not det-bounded")
        k = device.getKernel("PtShimTest", "SearchCheckKernel")
        launcher = adl.Launcher(device, k)
        launcher.setBuffers([adl.BufferInfo(b) for b in (t, r, m, o)])
        launcher.setConst(np.int64(36))              # (an 8-byte count)
        launcher.setConst(np.uint32(2))
        with pytest.raises(shim.ShimError) as e:
            launcher.launch1D(1)
        assert e.value.code == shim.PT_ERR_ARGS
        got = np.empty(2 * 512, np.uint32)
        o.read(got, 2 * 512)
        device.waitForCompletion()
        assert np.array_equal(got, sentinel), "a refused launch wrote results"
        # and the same buffers, asked properly: two waves of dead lanes with empty masks miss
        _launch(device, [t, r, m, o], 36, 2)
        o.read(got, 2 * 512)
        device.waitForCompletion()
        assert (got.reshape(-1, 8)[:, :4] == [0xFFFFFFFF, msc.MISS_T, 0, 0]).all()
    finally:
        for b in (t, r, m, o, nan, huge):
            b.release()


# ---- renders that reach the dense regime end to end ------------------------------------------------------------------------------
FRAMES, DEPTH = 4, 16
SHEETS = {"sheets": lambda: scenes.sheets(), "sheets_alternating": lambda: scenes.sheets(alternate=True)}


@pytest.fixture(scope="module")
def wanted(oracle):
    """the oracle's renders and accepted counts, each computed once"""
    cache = {}

    def get(name, W, H):
        if (name, W, H) not in cache:
            tris, mats = SHEETS[name]()
            with np.errstate(all="ignore"):
                want, st = oracle.render(tris, mats, W, H, FRAMES, max_bounces=DEPTH, want_stats=True)
            cache[name, W, H] = (tris, mats, want, st, msc.primary_accepted(tris, W, H, FRAMES))
        return cache[name, W, H]
    return get


def _primary_snapshot(device, expect_pixels):
    lib = shim.load()
    n = ctypes.c_uint32(0)
    rc = lib.pt_primary_mask_snapshot(device._h, ctypes.byref(n), None, 0)
    assert rc == 0, "no primary-mask table stands"
    assert n.value == expect_pixels
    out = np.zeros((n.value, 2), np.uint32)
    shim.check(lib.pt_primary_mask_snapshot(device._h, ctypes.byref(n), out.ctypes.data_as(ctypes.c_void_p), len(out)))
    return out


@pytest.mark.parametrize("masks", [1, 0])
@pytest.mark.parametrize("W,H", [(64, 64), (33, 97)])
@pytest.mark.parametrize("name", list(SHEETS))
def test_sheet_renders_match_the_oracle(device, wanted, name, W, H, masks):
    tris, mats, want, st, accepted = wanted(name, W, H)
    what = "%s, %d x %d, masks %d" % (name, W, H, masks)
    with options(device, PRIMARY_MASKS=masks, SECONDARY_MASKS=masks):
        got, gst = render(device, tris, mats, W, H, FRAMES, depth=DEPTH, want_stats=True)
        if masks:
            assert not no_table(device), what + ": no secondary-mask table stands"
            snap = _primary_snapshot(device, W * H)
            pop = np.unpackbits(snap.view(np.uint8)).sum() / (W * H)
            print("%s: primary masks hold %.2f triangles per pixel, the oracle accepts %.2f per primary ray" % (what, pop, accepted))
            assert pop >= accepted, what + ": the primary masks are sparser than the accepted sets they must contain"
    assert_fb_equal(got, want, what)
    assert gst[shim.PT_STAT_RAYS] == st["rays"], "%s: %d rays, the oracle traced %d" % (what, gst[shim.PT_STAT_RAYS], st["rays"])
    assert gst[shim.PT_STAT_SAMPLES] == st["samples"] == W * H * FRAMES
