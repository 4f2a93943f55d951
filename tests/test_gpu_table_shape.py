"""The shape of the secondary rays' table and the checkpoint regions that pay for it (GPU tier).

THE TABLE (csrc/pt_secmask.h: PT_SM_T tiles and PT_SM_C direction cells per edge; C may be odd, and 6 C^2 need not be a multiple of a
wave).  The device builds one entry per thread in a tile-major order of its own and the trace kernel finds an entry by multiplications
that used to be shifts, so for the smallest scene that has a table -- the box's floor, two triangles -- EVERY entry of the device's
table must equal the host build of the same function (tests/secondary_masks_check.cpp), 2 T^2 6 C^2 of them.  Scenes whose second mask
word is in use are compared at a prime stride that is neither the 211 nor the 1009 of the older tests and divides neither T^2 nor
6 C^2: 64 triangles (the largest byte offsets a table has) and 34 (two bits of the second word).  The count of entries is checked against
ntri T^2 6 C^2.  (A table of 33 triangles does not exist on the device: an odd count has no quad pairing, which
tests/test_gpu_secondary_masks_tight.py asserts; 34 is the nearest scene with a table.)

THE CHECKPOINTS.  A table kernel's wave stops by parking its live paths into its empty pool: at most PT_POOL = 56 records, and its
region of the carry buffer has room for exactly those (csrc/pt_kernels.h: PT_CARRY_HIT_RECORDS); the LBVH kernel's wave stores up to 64
shorter records into the same region.  Renders that stop at every frame must be bit-identical to the oracle, ray and sample counts
included, with PT_STAT_CARRIED above zero: the Cornell box at depth 16 and at 256 (the deepest the kernel with its table in LDS takes: its
pools fill), the same through the LBVH, and 288 triangles by brute force (the tiled kernel, whose record has 18 dwords)."""
import os
import subprocess

import numpy as np
import pytest

import scenes
from conftest import assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import scene as _scene, shim
from test_gpu_secondary_masks import no_table, snapshot
from test_gpu_secondary_masks_tight import TABLES
from test_secondary_masks_cpu import records
from test_secondary_masks_tight_cpu import one_quad

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STRIDE = 997


@pytest.fixture(scope="module")
def host_table(tmp_path_factory):
    d = tmp_path_factory.mktemp("secmask_shape_gpu")
    exe = str(d / "secondary_masks_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe,
                           os.path.join(HERE, "secondary_masks_check.cpp")])

    def table(tris, stride):
        rec, out = str(d / "records.f32"), str(d / "table.u32")
        records(tris).tofile(rec)
        subprocess.check_call([exe, "table", rec, str(len(tris)), out, str(stride)], stdout=subprocess.DEVNULL)
        return np.fromfile(out, np.uint32).reshape(-1, 2)
    return table


def _device_table(device, tris, mats, name):
    render(device, tris, mats, 16, 16, 1, depth=2)
    assert not no_table(device), name + ": no table stands"
    got, info = snapshot(device)
    T, C = info[2], info[3]
    assert info[1] == len(tris) and info[0] == len(got) == len(tris) * T * T * 6 * C * C, "%s: %d entries of %d triangles at T = %d, C = %d" % (
        name, len(got), len(tris), T, C)
    return got, T, C


def _assert_same(got, want, stride, name):
    assert len(got) == len(want), "%s: %d device entries, %d host entries" % (name, len(got), len(want))
    diff = np.flatnonzero((got != want).any(axis=1))
    assert len(diff) == 0, "%s: %d of %d entries differ (first: %d, device %s, host %s)" % (
        name, len(diff), len(want), diff[0] * stride, got[diff[0]], want[diff[0]])


def test_every_entry_of_the_smallest_table(device, host_table):
    tris, mats = one_quad(), _scene.load_model()[1]
    assert len(tris) == 2
    got, T, C = _device_table(device, tris, mats, "one quad")
    _assert_same(got, host_table(tris, 1), 1, "one quad")
    assert int(got[:, 1].max()) == 0 and int(got[:, 0].max()) <= 3, "bits above the scene's two triangles"


@pytest.mark.parametrize("name", ["sixty_four", "thirty_four"])
def test_the_second_mask_word_and_the_largest_offsets(device, host_table, name):
    tris, mats = TABLES[name]()
    assert len(tris) == {"sixty_four": 64, "thirty_four": 34}[name]
    got, T, C = _device_table(device, tris, mats, name)
    assert STRIDE not in (211, 1009) and (T * T) % STRIDE != 0 and (6 * C * C) % STRIDE != 0
    some = got[::STRIDE]
    _assert_same(some, host_table(tris, STRIDE), STRIDE, name)
    assert some[:, 1].any(), "no compared entry uses the second mask word"
    if len(tris) < 64:
        assert (got[:, 1] >> (len(tris) - 32)).max() == 0, "bits above the scene's triangles"


# ---- checkpoints at the regions' new capacity ----------------------------------------------------------------------------------------

def _assert_stops_at_every_frame(device, tris, mats, w, h, frames, depth, want, what, **opts):
    fb, ost = want
    with options(device, CHUNK_FRAMES=1, CHECKPOINT=1, **opts):
        got, st = render(device, tris, mats, w, h, frames, depth=depth, want_stats=True)
    assert_fb_equal(got, fb, what)
    assert int(st[shim.PT_STAT_RAYS]) == ost["rays"], "%s: %d rays, the oracle traced %d" % (what, int(st[shim.PT_STAT_RAYS]), ost["rays"])
    assert int(st[shim.PT_STAT_SAMPLES]) == ost["samples"] == w * h * frames, what
    assert int(st[shim.PT_STAT_CARRIED]) > 0, what + ": no path crossed a launch boundary"


@pytest.fixture(scope="module")
def cornell_64x64_f8(cornell, oracle):
    """the oracle's 64 x 64 images after 8 frames at depth 16 and 256, with their tallies: computed once, shared, never written"""
    tris, mats = cornell
    out = {}
    for depth in (16, 256):
        fb, st = oracle.render(tris, mats, 64, 64, 8, max_bounces=depth, want_stats=True)
        fb.setflags(write=False)
        out[depth] = (fb, st)
    return out


@pytest.mark.parametrize("accel", [0, 2])
@pytest.mark.parametrize("depth", [16, 256])
def test_the_box_stops_at_every_frame(device, cornell, cornell_64x64_f8, depth, accel):
    """accel 0: the kernel with its table in LDS, regions of PT_POOL 17-dword records; accel 2: the LBVH kernel, 64 records of 15 dwords"""
    tris, mats = cornell
    _assert_stops_at_every_frame(device, tris, mats, 64, 64, 8, depth, cornell_64x64_f8[depth],
                                 "the box, 8 one-frame launches, depth %d, PT_OPT_ACCEL %d" % (depth, accel), ACCEL=accel)


def test_the_tiled_kernel_stops_at_every_frame(device, oracle):
    tris, mats = scenes.nested_boxes(8)
    assert len(tris) > 256
    w, h, frames = 32, 32, 4
    want = oracle.render(tris, mats, w, h, frames, max_bounces=16, want_stats=True)
    assert int((want[0][:, :3] > 0).any(1).sum()) > w * h // 2, "the scene is not in view"
    _assert_stops_at_every_frame(device, tris, mats, w, h, frames, 16, want, "%d triangles by brute force, 4 one-frame launches" % len(tris), ACCEL=1)
