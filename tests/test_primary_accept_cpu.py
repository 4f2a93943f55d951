"""tests/primary_accept.c, the restatement the mask tests rely on, pinned to the CPU oracle: at max_bounces = 1 every ray the oracle
traces is a primary ray, so its tallies of accepted pairs and of pairs past the u test are the restatement's counts."""
import numpy as np
import pytest

import camera_oracle
import primary_accept
from oclpathtracer_amd.camera import Camera


@pytest.mark.parametrize("W,H,frames,frame_begin", [(48, 48, 4, 0), (33, 17, 3, 5)])
def test_counts_are_the_oracles(oracle, cornell, W, H, frames, frame_begin):
    tris, mats = cornell
    _, st = oracle.render(tris, mats, W, H, frames, frame_begin=frame_begin, max_bounces=1, want_stats=True)
    assert st["rays"] == W * H * frames
    acc, reach, n_acc, n_reach = primary_accept.union(tris, W, H, frames, frame_begin=frame_begin)
    assert n_acc == st["accept"]
    assert n_reach == st["rej_v"] + st["reach_t"]
    assert not (acc & ~reach).any(), "an accepted triangle that did not pass the u test"
    if W == H:   # the square view of the Cornell box: 1.20 accepted and 3.03 past u per primary ray (a wide view also sees past the box)
        assert 1.0 < n_acc / (W * H * frames) < 1.4 and 2.5 < n_reach / (W * H * frames) < 3.5


def test_counts_are_the_oracles_from_a_moved_camera(cornell):
    tris, mats = cornell
    cam = Camera((0.3, 1.5, -2.5), (0.0, 5.4, -2.8), up=(0.0, 0.0, -1.0))
    W, H, frames = 40, 24, 3
    _, st = camera_oracle.render(tris, mats, W, H, frames, cam, max_bounces=1, want_stats=True)
    _, _, n_acc, n_reach = primary_accept.union(tris, W, H, frames, cam=cam)
    assert n_acc == st["accept"] and n_reach == st["rej_v"] + st["reach_t"]


def test_a_pixel_subset_and_the_bit_order(cornell):
    tris, _ = cornell
    W, H = 16, 16
    acc, reach, _, _ = primary_accept.union(tris, W, H, 2)
    gid = np.array([5, 200, 17], np.int32)
    a2, r2, _, _ = primary_accept.union(tris, W, H, 2, gid=gid)
    assert np.array_equal(a2, acc[gid]) and np.array_equal(r2, reach[gid])
    # the device's table: triangle 32 c + j at bit n - 1 - j of word c
    snap = np.array([[1 << 31, 1 << 3], [1, 1]], np.uint32)   # 36 triangles: words of 32 and 4
    assert list(primary_accept.mask_bits(snap, 36)) == [1 | (1 << 32), (1 << 31) | (1 << 35)]
    assert list(primary_accept.popcount(np.array([0, 7, 1 << 63], np.uint64))) == [0, 3, 1]
