"""pt_shade's short forms return the bits of the literal operations (GPU tier).

The GGX branch of `pt_shade` forms its four quotients with one exact reciprocal and Markstein's correction while their
operands are in [2^-60, 2^60) (csrc/pt_device_math.h: pt_div, pt_div_by, pt_div_pair), and its two normalisations of vectors
that are unit vectors up to rounding take a form without a transcendental while a whole wave's squared lengths are within
2^-11 of 1 (pt_rsqrt_near1).  Here:

  * the forms against the literal operations ON THE GPU, operand by operand (pt_shade_check_kernel): 1 / sqrt over the whole
    window of the near-1 form, the reciprocal over every binary32 the quotients' guards admit, the guarded quotients over
    every pair of binades the guards admit and the first one outside on each side;
  * renders against the CPU oracle, bit for bit, of the Cornell box (r = 0.008: gd^2 reaches r^4 = 4.1e-9) and of a glossy
    room whose roughnesses lie on both sides of every edge of the guards that a roughness can reach.
"""
import numpy as np
import pytest

from conftest import assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import shim
from scenes import ROUGHNESS, glossy_room   # (the roughnesses on both sides of every guard edge: tests/scenes.py)

pytestmark = pytest.mark.gpu

BINADES, SIGS = 122, 4096   # PT_SHADE_CHECK_BINADES, PT_SHADE_CHECK_SIGS (csrc/pt_kernels.hip)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _check(device, mode, first, count):
    from oclpathtracer_amd import adl

    k = device.getKernel("PtShimTest", "ShadeCheckKernel")
    assert k is not None
    out = adl.Buffer(device, 8, np.uint64)
    try:
        out.write(np.zeros(8, np.uint64), 8)
        launcher = adl.Launcher(device, k)
        launcher.setBuffers([adl.BufferInfo(out)])
        launcher.setConst(np.int32(mode))
        launcher.setConst(np.uint32(first))
        launcher.setConst(np.uint64(count))
        launcher.launch1D(1)
        res = np.empty(8, np.uint64)
        out.read(res, 8)
        device.waitForCompletion()
    finally:
        out.release()
    return [int(v) for v in res]


def test_near_one_form_equals_the_two_roundings_over_its_window(device):
    """mode 1: every binary32 within 2^-11 of 1 against 1.0f / sqrtf(x) (the CPU tier runs the same: tests/test_shade_near1_cpu.py)"""
    lo, hi = _bits(1.0 - 2.0 ** -11), _bits(1.0 + 2.0 ** -11)
    res = _check(device, 1, lo - 64, hi - lo + 1 + 128)     # (and 64 values on each side, which the kernel must leave out)
    print("1/sqrt near 1: %d operands, %d mismatches" % (res[4], res[1]))
    assert res[4] == hi - lo + 1 == 12289
    assert res[1] == 0


def test_reciprocal_is_exact_over_the_quotients_window(device):
    """mode 3: every binary32 of [2^-60, 1e20] -- the window of the guarded quotients' divisors and the range pt_rcp already
    relied on -- against 1.0f / x"""
    lo, hi = _bits(2.0 ** -60), _bits(1e20)
    res = _check(device, 3, lo, hi - lo + 1)
    print("1/x: %d operands, %d mismatches" % (res[4], res[3]))
    assert res[4] == hi - lo + 1
    assert res[3] == 0


def test_guarded_quotients_equal_ieee_division_on_both_sides_of_every_guard(device):
    """mode 2: 122 x 122 pairs of binades (2^-61 .. 2^60), 4096 pairs of significands each -- all zeros and all ones among
    them, and a +0 numerator"""
    res = _check(device, 2, 20261018, BINADES * BINADES * SIGS)
    print("quotients: %d operand pairs, %d inside the window, %d mismatches" % (res[4], res[5], res[2]))
    assert res[4] == BINADES * BINADES * SIGS
    assert res[5] == (BINADES - 2) * (BINADES - 2) * (SIGS - 1)   # (the +0 numerator is outside it)
    assert res[2] == 0


def test_smallest_roughness_with_a_normal_fourth_power():
    r = np.float32(ROUGHNESS[2])
    tiny = np.float32(np.finfo(np.float32).tiny)
    with np.errstate(under="ignore"):
        assert (r * r) * (r * r) >= tiny
        below = np.nextafter(r, np.float32(0.0))
        assert (below * below) * (below * below) < tiny


@pytest.fixture(scope="module")
def wanted(oracle, cornell):
    """the oracle's renders, once: 64 x 48, 8 frames, depth 16"""
    with np.errstate(all="ignore"):
        return {name: (t, m) + tuple(oracle.render(t, m, 64, 48, 8, max_bounces=16, want_stats=True))
                for name, (t, m) in (("cornell", cornell), ("glossy_room", glossy_room()))}


@pytest.mark.parametrize("accel", [0, 2])
@pytest.mark.parametrize("name", ["cornell", "glossy_room"])
def test_render_matches_the_oracle(device, wanted, name, accel):
    """through the table kernel (36 triangles: PT_OPT_ACCEL = 0 searches the LDS table) and the LBVH (PT_OPT_ACCEL = 2)"""
    tris, mats, want, st = wanted[name]
    with options(device, ACCEL=accel):
        got, gst = render(device, tris, mats, 64, 48, 8, depth=16, want_stats=True)
    assert_fb_equal(got, want, "%s, accel %d" % (name, accel))
    assert gst[shim.PT_STAT_RAYS] == st["rays"]
    assert gst[shim.PT_STAT_SAMPLES] == st["samples"] == 64 * 48 * 8
