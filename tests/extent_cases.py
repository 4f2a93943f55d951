"""The inputs of tests/test_gpu_extents.py -- images and frame numbers at the ends of what the C ABI accepts -- and what the CPU oracle
says of them: one table, so that tests/test_extents_cpu.py proves on exactly the geometries the device renders that each reaches the
corner it is rendered for.  TEST INFRASTRUCTURE.

  TALL   64 x (2^25 - 1): W * H = 2 147 483 584, the last multiple of 64 the ABI accepts.  A rank of a striped render owns a few rows
         however tall the image is: the layouts below have 448 .. 1 984 local pixels, whose global rows, gids and seeds use all 31 bits.
  WIDE   (2^24 + 256) x 127, one row of it: the columns about the image's centre, where the box is, lie at and above 2^23, where
         binary32 has spacing 1 and a jittered x is a neighbouring column's.
  LATE   the Cornell box at 24 x 16 resumed at frame numbers about 2048 (the fold's reciprocal table ends), 2^24 (the float of a
         frame number and of its predecessor coincide) and 2^31 - 1 (the last frame the ABI accepts).
  EMPTY  a rank that owns no row."""
from __future__ import annotations

import numpy as np

import direct_oracle as do
import extent_oracle as eo
import indirect_oracle as io
import roulette_oracle as ro
from scenes import edge_scene

# ---- TALL -------------------------------------------------------------------------------------------------------------------------
TALL_W, TALL_H = 64, 2 ** 25 - 1
TALL_FRAMES = 3
# name -> the stripe layout.  "last_pixel": rows rank + k 2^22, k = 0 .. 7 -- 8 rows, the last one the image's last;  "ragged": k = 7
# would be row 2^25 - 1 = H, 7 rows;  "stripes_of_3": the image's last row, 2^25 - 2 = 3 * 11 184 810, begins stripe 11 184 810 =
# 10 * 2^20 + 699 050 -- ten whole stripes and a stripe of one row, 31 rows
TALL = {
    "last_pixel": dict(stripe_rows=1, n_ranks=2 ** 22, rank=2 ** 22 - 2),
    "ragged": dict(stripe_rows=1, n_ranks=2 ** 22, rank=2 ** 22 - 1),
    "stripes_of_3": dict(stripe_rows=3, n_ranks=2 ** 20, rank=699050),
}
TALL_ROWS = {"last_pixel": 8, "ragged": 7, "stripes_of_3": 31}

# ---- WIDE -------------------------------------------------------------------------------------------------------------------------
WIDE_W, WIDE_H = 2 ** 24 + 256, 127
WIDE_STRIPES = dict(stripe_rows=1, n_ranks=127, rank=40)   # one local row, global row 40
WIDE_ROW = 40
WIDE_FRAMES = 8
WIDE_MASK_FRAMES = 32                                       # the masks' superset is checked over frames 0 .. 31

# ---- LATE -------------------------------------------------------------------------------------------------------------------------
LATE_W, LATE_H = 24, 16
LATE = {"table_end": (2046, 5), "float_ties": (2 ** 24 - 2, 5), "last_frames": (2 ** 31 - 4, 3)}   # name -> (frame_begin, frames)

# ---- EMPTY ------------------------------------------------------------------------------------------------------------------------
EMPTY_W, EMPTY_H = 7, 5
EMPTY_STRIPES = dict(stripe_rows=4, n_ranks=3, rank=2)

# ---- the lit estimators: name -> (max_bounces or None for direct, mis, power, roulette (R, cap) or None) ---------------------------
LIT_K, LIT_B = 1, 6
LIT = {"direct": (None, False, False, None), "indirect": (LIT_B, False, False, None), "mis_power_rr": (LIT_B, True, True, (1, 0.5))}
LIT_FRAMES = 2     # of a TALL lit render

# (H, stripe_rows, n_ranks, rank) of the layouts tests elsewhere in the suite render or restate (the closed forms of direct_oracle
# must give what the walk over the rows gave)
EXISTING_LAYOUTS = [(16, 1, 1, 0), (24, 1, 1, 0), (64, 16, 1, 0), (31, 5, 1, 0), (31, 5, 3, 0), (31, 5, 3, 1), (31, 5, 3, 2),
                    (16, 3, 3, 0), (16, 3, 3, 1), (16, 3, 3, 2), (30, 4, 3, 1), (48, 8, 4, 1), (33, 4, 2, 0), (33, 4, 2, 1),
                    (24, 16, 3, 1), (8, 4, 8, 3), (64, 16, 2, 1), (40, 16, 8, 2), (40, 16, 8, 3), (47, 5, 3, 0), (5, 4, 3, 2)]


def cornell():
    """(tris, mats, lights, None): the Cornell box, the reference's camera"""
    return edge_scene("cornell")[1]


def tall_gids(name):
    return do.local_gids(TALL_W, TALL_H, **TALL[name])


def wide_columns():
    """the columns of the WIDE row that are read back and compared, as (name, first column, count) blocks and one array of 4 096
    single columns drawn once with a fixed seed: the window about the image's centre (where the box is), both ends of the row, and
    columns all over it"""
    blocks = [("window", WIDE_W // 2 - 128, 257), ("first", 0, 64), ("last", WIDE_W - 64, 64)]
    scattered = np.sort(np.random.default_rng(20261019).choice(WIDE_W, 4096, replace=False)).astype(np.int64)
    return blocks, scattered


def wide_gids(cols):
    return WIDE_ROW * WIDE_W + np.asarray(cols, np.int64)


def window_columns():
    _, first, n = wide_columns()[0][0]
    return np.arange(first, first + n, dtype=np.int64)


def late_start(channels=4):
    """a framebuffer of arbitrary finite values in [0, 1] to resume from, float32 [pixels, 4]"""
    return np.random.default_rng(2048).uniform(0.0, 1.0, (LATE_W * LATE_H, channels)).astype(np.float32)


# ---- what the oracles say: computed once, shared, read-only ---------------------------------------------------------------------
def _fused_window(W, H, frames, frame_begin, depth, gid_key, start_key):
    tris, mats = cornell()[:2]
    gid = _GIDS[gid_key]()
    start = late_start() if start_key else None
    px, st = eo.render_window(tris, mats, W, H, frames, gid, frame_begin=frame_begin, max_bounces=depth, start=start)
    return px, np.array([st["rays"], st["samples"]], np.uint64)


def _wide_all():
    blocks, scattered = wide_columns()
    return wide_gids(np.concatenate([np.arange(f, f + n) for _, f, n in blocks] + [scattered]))


_GIDS = {("tall", name): (lambda name=name: tall_gids(name)) for name in TALL}
_GIDS["late"] = lambda: np.arange(LATE_W * LATE_H)
_GIDS["wide"] = _wide_all


def fused_tall(name):
    """(pixels [local pixels, 4], [rays, samples]) of TALL_FRAMES frames of a TALL layout"""
    return do.once(_fused_window, TALL_W, TALL_H, TALL_FRAMES, 0, 16, ("tall", name), False)


def fused_late(name):
    fb, n = LATE[name]
    return do.once(_fused_window, LATE_W, LATE_H, n, fb, 16, "late", True)


def fused_wide():
    """the pixels of wide_columns(), blocks first and in their order, then the scattered columns"""
    return do.once(_fused_window, WIDE_W, WIDE_H, WIDE_FRAMES, 0, 16, "wide", False)


def _lit(est, W, H, frames, frame_begin, late, **stripes):
    tris, mats, lights, cam = cornell()
    B, mis, power, rr = LIT[est]
    start = late_start() if late else None
    gid, frame = do.sample_ids(W, H, frames, **stripes)
    frame = frame + frame_begin
    assert gid.max() < 2 ** 31 and frame.max() < 2 ** 31
    if B is None:
        fb = do.render(tris, mats, W, H, frame_begin, frames, LIT_K, lights=lights, cam=cam, start=start, **stripes)
        rad = do.decisions(tris, mats, W, H, gid, frame, LIT_K, lights=lights, cam=cam)[2]
    elif rr is None:
        fb = io.render(tris, mats, W, H, frame_begin, frames, LIT_K, B, lights=lights, cam=cam, start=start, **stripes)
        rad = io.samples(tris, mats, W, H, gid, frame, LIT_K, B, lights=lights, cam=cam)[0]
    else:
        fb = ro.render(tris, mats, W, H, frame_begin, frames, LIT_K, B, rr[0], rr[1], mis=mis, power=power, lights=lights, cam=cam,
                       start=start, **stripes)
        rad = ro.samples(tris, mats, W, H, gid, frame, LIT_K, B, rr[0], rr[1], mis=mis, power=power, lights=lights, cam=cam)[0]
    return fb, rad.reshape(frames, -1, 3)


def lit_tall(est, name):
    """the restatement's (framebuffer [local pixels, 4], radiance [frames, local pixels, 3]) of a lit estimator on a TALL layout"""
    return do.once(_lit, est, TALL_W, TALL_H, LIT_FRAMES, 0, False, **TALL[name])


def lit_late(est, name):
    fb, n = LATE[name]
    return do.once(_lit, est, LATE_W, LATE_H, n, fb, True)
