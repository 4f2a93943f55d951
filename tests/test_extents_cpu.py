"""The extremes of image size and frame number on the CPU: the proof that every geometry of tests/extent_cases.py reaches the corner
tests/test_gpu_extents.py renders it for, and the checks of the oracle support those tests lean on.  No GPU.

  - TALL: the layouts' local rows are what the table says, their gids reach W * H - 1 and need all 31 bits, and their primary rays
    hit at least three different triangles (an image of misses would compare nothing but the background);
  - WIDE: over its 8 frames the window about the image's centre holds samples whose ray lies further from the pixel's centre ray
    than the eps of pt_primary_mask_kernel allows -- the premise of the masks' footprint bound is broken there -- and pixels whose
    union of accepted triangles has two members or more, so that a wrong mask has something to drop;
  - LATE: the frames include z with (float)(z - 1) == (float)z, a pair on either side of 2048, and the last frame the ABI accepts;
  - the windowed render (tests/extent_oracle.c) is ptoracle.render at the listed pixels, bit for bit, tallies included;
  - the closed forms of direct_oracle's row helpers are the walk over the rows they replace, on every layout the suite uses and on
    every small one; pt_local_rows (the shim loads without a GPU) is the same closed form up to 2^31 - 1."""
import numpy as np
import pytest

import direct_oracle as do
import extent_cases as xc
import extent_oracle as eo
import primary_accept
from conftest import assert_fb_equal
from oracle import ptoracle

F = np.float32


# ---- the row helpers ---------------------------------------------------------------------------------------------------------------
def _walk(H, sr, nr, rank):
    return [r for r in range(H) if (r // sr) % nr == rank]


def test_closed_forms_are_the_walk_over_the_rows():
    layouts = list(xc.EXISTING_LAYOUTS) + [(H, sr, nr, rank) for H in (1, 2, 5, 17, 40) for sr in (1, 2, 3, 6) for nr in (1, 2, 5)
                                           for rank in range(nr)]
    for H, sr, nr, rank in layouts:
        rows = _walk(H, sr, nr, rank)
        what = "H %d stripe_rows %d n_ranks %d rank %d" % (H, sr, nr, rank)
        assert do.local_row_count(H, sr, nr, rank) == len(rows), what
        assert do.local_rows(H, sr, nr, rank).tolist() == rows, what
        W = 3
        want = (np.asarray(rows, np.int64)[:, None] * W + np.arange(W)[None, :]).reshape(-1)
        assert np.array_equal(do.local_gids(W, H, stripe_rows=sr, n_ranks=nr, rank=rank), want), what
        gid, frame = do.sample_ids(W, H, 2, stripe_rows=sr, n_ranks=nr, rank=rank)
        assert np.array_equal(gid, np.tile(want, 2)) and np.array_equal(frame, np.repeat(np.arange(2), len(want))), what


def test_pt_local_rows_is_the_closed_form():
    """the layouts of the table, every small layout, and 400 random ones up to 2^31 - 1"""
    from oclpathtracer_amd import shim

    lib = shim.load()
    M = 2 ** 31 - 1
    cases = [(xc.TALL_H, s["stripe_rows"], s["n_ranks"], s["rank"]) for s in xc.TALL.values()]
    cases += [(xc.WIDE_H, 1, 127, 40), (xc.EMPTY_H, 4, 3, 2), (M, 1, 1, 0), (M, M, 1, 0), (M, 1, M, M - 1), (M, 1, M, 0), (M, M, M, M - 1),
              (M, 2, 2 ** 30, 2 ** 30 - 1), (M, 2 ** 16, 2 ** 15, 2 ** 15 - 1), (0, 1, 1, 0)]
    cases += list(xc.EXISTING_LAYOUTS)
    rng = np.random.default_rng(31)
    for _ in range(400):
        H = int(rng.integers(1, M, endpoint=True)) if rng.uniform() < 0.5 else int(2 ** rng.uniform(0, 31))
        sr = int(min(M, 2 ** rng.uniform(0, 31)))
        nr = int(min(M, 2 ** rng.uniform(0, 31)))
        rank = int(rng.integers(0, nr)) if rng.uniform() < 0.7 else (H // sr) % nr   # (often the rank of the image's last stripe)
        cases.append((H, sr, nr, rank))
    for H, sr, nr, rank in cases:
        got = lib.pt_local_rows(H, sr, nr, rank)
        assert got == do.local_row_count(H, sr, nr, rank), "pt_local_rows(%d, %d, %d, %d) = %d" % (H, sr, nr, rank, got)
    for name, s in xc.TALL.items():
        assert lib.pt_local_rows(xc.TALL_H, s["stripe_rows"], s["n_ranks"], s["rank"]) == xc.TALL_ROWS[name]
    e = xc.EMPTY_STRIPES
    assert lib.pt_local_rows(xc.EMPTY_H, e["stripe_rows"], e["n_ranks"], e["rank"]) == 0


# ---- the windowed render -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_begin", [0, 7, 2046])
def test_windowed_render_is_the_oracles_render(frame_begin):
    tris, mats = xc.cornell()[:2]
    W, H, frames = 20, 12, 4
    start = np.random.default_rng(5).uniform(0, 1, (W * H, 4)).astype(np.float32)
    want, st = ptoracle.render(tris, mats, W, H, frames, frame_begin=frame_begin, fb=start.copy(), want_stats=True)
    gid = np.random.default_rng(6).permutation(W * H)
    got, gst = eo.render_window(tris, mats, W, H, frames, gid, frame_begin=frame_begin, start=start[gid])
    assert_fb_equal(got, want[gid], "frames from %d" % frame_begin)
    assert gst == st
    some = gid[:37]
    got, gst = eo.render_window(tris, mats, W, H, frames, some, frame_begin=frame_begin, start=start[some], max_bounces=3)
    want3, st3 = ptoracle.render(tris, mats, W, H, frames, frame_begin=frame_begin, fb=start.copy(), max_bounces=3, want_stats=True)
    assert_fb_equal(got, want3[some], "37 pixels, 3 bounces")
    assert gst["samples"] == 37 * frames and 0 < gst["rays"] < st3["rays"]
    with pytest.raises(AssertionError):
        eo.render_window(tris, mats, W, H, 1, [W * H])


# ---- TALL --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(xc.TALL))
def test_tall_layouts_reach_the_last_pixels(name):
    s = xc.TALL[name]
    rows = do.local_rows(xc.TALL_H, **s)
    assert len(rows) == xc.TALL_ROWS[name] and rows.max() < xc.TALL_H
    assert ((rows // s["stripe_rows"]) % s["n_ranks"] == s["rank"]).all()
    gid = xc.tall_gids(name)
    assert xc.TALL_W * xc.TALL_H == 2 ** 31 - 64 and gid.max() < 2 ** 31
    if name == "ragged":
        assert rows.max() + s["n_ranks"] == xc.TALL_H, "the next period's row is not the first one outside the image"
        assert gid.max() >= 2 ** 30
    else:
        assert gid.max() == xc.TALL_W * xc.TALL_H - 1, "the layout does not reach the image's last pixel"
    assert rows.max() >= 2 ** 24, "no row above the exact floats"


@pytest.mark.parametrize("name", list(xc.TALL))
def test_tall_primary_rays_hit_the_scene(name):
    tris, mats = xc.cornell()[:2]
    gid = xc.tall_gids(name)
    g = np.tile(gid, xc.TALL_FRAMES).astype(np.int32)
    f = np.repeat(np.arange(xc.TALL_FRAMES), len(gid)).astype(np.int32)
    _, hits = ptoracle.paths(tris, mats, g, f, xc.TALL_W, xc.TALL_H, max_bounces=1)
    first = hits[:, 0]
    assert len(np.unique(first[first >= 0])) >= 3, "the primary rays hit %s" % np.unique(first)
    px, st = xc.fused_tall(name)
    assert st[1] == len(gid) * xc.TALL_FRAMES and st[0] > 2 * st[1], "paths of fewer than two rays on average"


# ---- WIDE --------------------------------------------------------------------------------------------------------------------------
def _mask_eps():
    """eps of pt_primary_mask_kernel for the WIDE image and the reference camera, in its float operations"""
    angle = F(float.fromhex("0x1.279a74p-1"))
    hx = angle * (F(xc.WIDE_W) / F(xc.WIDE_H)) / F(xc.WIDE_W)
    hy = angle / F(xc.WIDE_H)
    return F(np.sqrt(hx * hx + hy * hy)) * F(1.01) + F(4e-6)


def _centre_dir(x, y):
    """the mask kernel's centre ray of pixel (x, y): pt_camera_ray at the jitter's midpoint, the image-plane point in float as the
    kernel forms it, the normalisation in double (its float roundings are 1e-7, eps is 6.5e-3)"""
    W, H = xc.WIDE_W, xc.WIDE_H
    angle = F(float.fromhex("0x1.279a74p-1"))
    inv_w, inv_h, aspect = F(1) / F(W), F(1) / F(H), F(W) / F(H)
    X = (F(2) * ((F(x) + F(.5)) * inv_w) - F(1)) * angle * aspect
    Y = -(F(1) - F(2) * ((F(y) + F(.5)) * inv_h)) * angle
    d = np.array([X, -Y, -1.0], np.float64)
    return d / np.linalg.norm(d)


def test_wide_window_breaks_the_footprint_premise():
    assert xc.WIDE_W * xc.WIDE_H < 2 ** 31 and xc.window_columns().min() >= 2 ** 23
    eps = float(_mask_eps())
    far = total = 0
    worst = 0.0
    for x in xc.window_columns():
        dc = _centre_dir(int(x), xc.WIDE_ROW)
        gid = xc.WIDE_ROW * xc.WIDE_W + int(x)
        for frame in range(xc.WIDE_FRAMES):
            _, d, _ = ptoracle.generate_ray(int(x), xc.WIDE_ROW, xc.WIDE_W, xc.WIDE_H, gid + ptoracle.hash_u32(frame))
            dist = float(np.abs(d.astype(np.float64) - dc).max())
            worst = max(worst, dist)
            far += dist > eps
            total += 1
    print("eps %.5f; %d of %d samples lie further from the centre ray in some component, the furthest %.5f" % (eps, far, total, worst))
    assert far > 0, "every sample of the window lies within eps of its pixel's centre ray: the masks' premise holds here"


def test_wide_window_pixels_have_several_candidates():
    tris = xc.cornell()[0]
    gid = xc.wide_gids(xc.window_columns())
    acc, _, _, _ = primary_accept.union(tris, xc.WIDE_W, xc.WIDE_H, xc.WIDE_FRAMES, gid=gid)
    pop = primary_accept.popcount(acc)
    assert (pop >= 2).any(), "no pixel of the window has two accepted triangles over the frames rendered"
    assert (pop >= 1).sum() > 128, "the box covers %d pixels of the window" % int((pop >= 1).sum())
    px, st = xc.fused_wide()
    assert len(px) == 257 + 64 + 64 + 4096 and st[1] == len(px) * xc.WIDE_FRAMES


# ---- LATE --------------------------------------------------------------------------------------------------------------------------
def test_late_frames_reach_their_edges():
    z = {name: np.arange(fb, fb + n, dtype=np.int64) for name, (fb, n) in xc.LATE.items()}
    t = z["table_end"]
    assert 2047 in t and 2048 in t and t.min() < 2047 and t.max() > 2048      # the table's last entry, the first division
    ties = z["float_ties"]
    assert any(F(int(k) - 1) == F(int(k)) for k in ties) and any(F(int(k) - 1) != F(int(k)) for k in ties)
    last = z["last_frames"]
    assert last.max() + 1 == 2 ** 31 - 1 and xc.LATE["last_frames"][0] + xc.LATE["last_frames"][1] == 2 ** 31 - 1
    start = xc.late_start()
    assert np.isfinite(start).all() and start.min() >= 0.0 and start.max() <= 1.0
    for name in xc.LATE:
        px, st = xc.fused_late(name)
        assert not np.array_equal(px[:, :3], start[:, :3]) or name != "table_end", "five frames at z = 2046 left the image as it was"
        assert st[1] == xc.LATE_W * xc.LATE_H * xc.LATE[name][1]


def test_empty_rank_owns_no_row():
    assert do.local_row_count(xc.EMPTY_H, **xc.EMPTY_STRIPES) == 0 and len(do.local_gids(xc.EMPTY_W, xc.EMPTY_H, **xc.EMPTY_STRIPES)) == 0


@pytest.mark.parametrize("est", list(xc.LIT))
def test_lit_tall_samples_carry_light(est):
    """the lit restatements take the TALL gids and late frames as they are, and their samples are not all background or black"""
    fb, rad = xc.lit_tall(est, "last_pixel")
    assert rad.shape == (xc.LIT_FRAMES, 512, 3) and fb.shape == (512, 4)
    assert len(np.unique(rad.reshape(-1, 3), axis=0)) > 64, "fewer than 65 different radiances in 1 024 samples"
    lfb, lrad = xc.lit_late(est, "last_frames")
    assert lrad.shape == (3, xc.LATE_W * xc.LATE_H, 3) and np.isfinite(lfb).all()
