"""Light lists and selection tables at scale and at their numeric edges on the MI355X, bit for bit.

tests/test_gpu_power.py and tests/test_gpu_mis.py stop at lists of 214 entries rendered and 70 020 entries built, a table total of
1 852 014 996 and three emission levels of one room.  Here pt_light_table is compared with tests/power_oracle.c -- cdf[0 .. nl] and tri_q
-- where the total passes 2^32 (from 65 537 entries on), where pt_light_tiles_kernel's threads own more than one tile (from 524 289
entries on), at the longest list the ABI accepts (2^24 - 1 entries, a total of up to 2^40 - 65536) and on every list of
power_scenes.power_sweep (powers from the subnormals to overflow, NaN, infinities, material indices out of range); pt_light_counts
with np.bincount at those lengths; and every lit estimator -- direct, indirect, MIS, by power and with the uniform choice -- with its
restatement on lists of 524 289 and 2^24 - 1 entries: the sample workspace with the radiance before the fold, and the framebuffer, NaN
masks equal.  tests/test_power_cpu.py proves, on these very inputs, what they reach."""
import numpy as np
import pytest

import power_cases as pc
import power_oracle as po
import power_scenes as ps
from conftest import assert_fb_equal
from gpu_support import lit_with_samples, options
from oclpathtracer_amd import scene, shim
from power_support import assert_table, power_with_samples

pytestmark = pytest.mark.gpu

W, H, FRAMES = pc.W, pc.H, pc.FRAMES
MODES = pytest.mark.parametrize("mode", pc.MODES, ids=[pc.MODE_NAMES[m] for m in pc.MODES])
BLOCK, TILE = 256, 2048   # csrc/pt_kernels.h: PT_LIGHT_SCAN_BLOCK, PT_LIGHT_SCAN_TILE


# ---- the table -------------------------------------------------------------------------------------------------------------------
def test_table_of_the_shortest_list_whose_total_passes_two_to_the_32(device):
    ut, um = ps.unequal_lights()
    li = ps.panel_heavy_list(65537)
    cdf, _ = assert_table(device, ut, um, li, "65 537 entries, all but one a panel triangle")
    assert int(cdf[-1]) == (1 << 32) + 1                             # 65 536 entries of q = 65536 and one of q = 1


@pytest.mark.parametrize("nl", [BLOCK * TILE - 1, BLOCK * TILE, BLOCK * TILE + 1, 2 * BLOCK * TILE + 3])
def test_table_sizes_about_one_tile_per_thread(device, nl):
    """256 tiles, the last one short or full; 257: two per thread, the 129th thread with one and the rest with none; 513: three per
    thread, the last thread with a partial share"""
    ut, um = ps.unequal_lights()
    cdf, _ = assert_table(device, ut, um, ps.long_list(nl), "nl = %d" % nl)
    assert int(cdf[-1]) >= 1 << 32


def test_table_of_the_longest_list(device):
    ut, um = ps.unequal_lights()
    want = pc.table_of("unequal", "max")
    assert_table(device, ut, um, pc.lights_of("unequal", "max"), "2^24 - 1 entries", want=want[:2])


def test_table_of_the_largest_total(device):
    ut, um = ps.unequal_lights()
    want = pc.table_of("unequal", "panels")
    cdf, tri_q = assert_table(device, ut, um, pc.lights_of("unequal", "panels"), "2^24 - 1 panel entries", want=want[:2])
    assert np.array_equal(cdf, np.arange(ps.MAX + 1, dtype=np.uint64) * np.uint64(65536)) and int(cdf[-1]) == (1 << 40) - 65536
    assert int(tri_q[10]) == 65536 and int(tri_q.astype(np.int64).sum()) == 65536


def test_table_of_every_list_of_the_power_sweep(device):
    tris, mats, lists = ps.power_sweep()
    for name, li in lists.items():
        assert_table(device, tris, mats, li, "power sweep, list %s" % name)


def test_a_short_table_rebuilt_into_a_long_ones_buffers(device):
    from oclpathtracer_amd import adl

    ut, um = ps.unequal_lights()
    long_list, short_list = pc.lights_of("unequal", "long"), scene.emitters(ut, um)[::-1].astype(np.int32)
    tables = (adl.Buffer(device, shim.load().pt_light_table_bytes(len(long_list)) // 8, np.uint64), adl.Buffer(device, len(ut), np.uint32))
    try:
        assert_table(device, ut, um, long_list, "524 289 entries", want=pc.table_of("unequal", "long")[:2], tables=tables)
        for li in (short_list, ps.zero_list()):
            assert_table(device, ut, um, li, "%d entries into the same buffers" % len(li), tables=tables)
    finally:
        for b in tables:
            b.release()


# ---- the counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["long", "max", "panels"])
def test_counts_of_the_long_lists(device, name):
    """pt_light_counts against np.bincount; the all-panel list puts 2^24 - 1 atomic adds on one counter"""
    from oclpathtracer_amd import adl

    li, ntri = pc.lights_of("unequal", name), len(ps.unequal_lights()[0])
    want = np.bincount(np.clip(li, 0, ntri - 1), minlength=ntri).astype(np.int32)
    lb, cb = adl.Buffer(device, len(li), np.int32), adl.Buffer(device, ntri, np.int32)
    try:
        lb.write(li, len(li))
        cb.write(np.full(ntri, -7, np.int32), ntri)
        assert shim.load().pt_light_counts(device._h, lb._h, len(li), ntri, cb._h, None) == shim.PT_OK
        got = np.zeros(ntri, np.int32)
        cb.read(got, ntri)
        device.waitForCompletion()
    finally:
        lb.release()
        cb.release()
    assert np.array_equal(got, want), "list %s: counts differ at %s" % (name, np.flatnonzero(got != want)[:4])
    assert np.array_equal(want, pc.table_of("unequal", name)[2]) and int(want.sum()) == len(li)


# ---- renders against the restatement ---------------------------------------------------------------------------------------------
def _compare(device, mode, lights, Ws, Hs, frames, what, power=True):
    K, B = pc.LONG_KB
    tris, mats, cam = pc.scene_of("unequal")
    sc = (tris, mats, pc.lights_of("unequal", lights), cam)
    what = "%s, %s choice, list %s, %s" % (pc.MODE_NAMES[mode], "power" if power else "uniform", lights, what)
    if power:
        want_fb, want_rad = pc.wanted(mode, "unequal", lights, Ws, Hs, frames, K, B)
        fb, ws = power_with_samples(device, mode, sc, Ws, Hs, frames, K, B)
    else:
        want_fb, want_rad = pc.wanted_uniform(mode, "unequal", lights, Ws, Hs, frames, K, B)
        fb, ws = lit_with_samples(device, sc, Ws, Hs, frames, K, max_bounces=None if mode == po.DIRECT else B, mis=mode == po.MIS)
    assert_fb_equal(ws[:frames], want_rad, what + ": radiance before the fold")
    assert_fb_equal(fb, want_fb, what)


@MODES
@pytest.mark.parametrize("power", [True, False], ids=["power", "uniform"])
def test_a_list_of_257_tiles(device, mode, power):
    """524 289 entries, a total of 9 692 185 602: the choice reads cdf values above 2^32 and entries above 2^16; the MIS estimator
    counts of 75 354.  The uniform choice reads the same list"""
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            _compare(device, mode, "long", W, H, FRAMES, "accel %d" % accel, power)


@MODES
@pytest.mark.parametrize("power", [True, False], ids=["power", "uniform"])
def test_a_list_of_257_tiles_on_a_small_image(device, mode, power):
    Ws, Hs = pc.LONG_SMALL
    for accel in (1, 2):
        with options(device, ACCEL=accel):
            _compare(device, mode, "long", Ws, Hs, FRAMES, "%dx%d accel %d" % (Ws, Hs, accel), power)


def test_direct_by_power_at_the_largest_total(device):
    """2^24 - 1 panel entries: x = (u total) >> 24 with total = 2^40 - 65536, the bound behind "the product stays below 2^64\""""
    _compare(device, po.DIRECT, "panels", W, H, pc.MAX_FRAMES, "2^24 - 1 entries")


@pytest.mark.parametrize("power", [True, False], ids=["power", "uniform"])
def test_mis_on_the_longest_list(device, power):
    """2^24 - 1 entries: a search of 24 levels and counts of 2 395 665 by power; (unsigned)(r0 * nl) beyond 2^23, where the product's ulp
    is 1, with the uniform choice"""
    _compare(device, po.MIS, "max", W, H, pc.MAX_FRAMES, "2^24 - 1 entries", power)
