"""The extremes of image size and frame number on the CPU: the proof that every geometry of tests/extent_cases.py reaches the corner
tests/test_gpu_extents.py and tests/test_gpu_extents_lists.py render it for, and the checks of the oracle support those tests lean on.
No GPU.

  - TALL: the layouts' local rows are what the table says, their gids reach W * H - 1 and need all 31 bits, and their primary rays
    hit at least three different triangles (an image of misses would compare nothing but the background);
  - WIDE: over its 8 frames the window about the image's centre holds samples whose ray lies further from the pixel's centre ray
    than the eps of pt_primary_mask_kernel allows -- the premise of the masks' footprint bound is broken there -- and pixels whose
    union of accepted triangles has two members or more, so that a wrong mask has something to drop;
  - LATE: the frames include z with (float)(z - 1) == (float)z, a pair on either side of 2048, and the last frame the ABI accepts;
  - the windowed render (tests/extent_oracle.c) is ptoracle.render at the listed pixels, bit for bit, tallies included;
  - the closed forms of direct_oracle's row helpers are the walk over the rows they replace, on every layout the suite uses and on
    every small one; pt_local_rows (the shim loads without a GPU) is the same closed form up to 2^31 - 1;
  - the entry points added since (RIS, environment, lens, features, pixel lists): the primary rays of the new TALL cases hit and miss;
    RIS keeps a candidate other than the first; environment samples contribute and a weighted ray leaves the scene; the lens rays are
    not the pinhole's; the WIDE list's window has hits and a sample whose jittered column is a neighbour's; the wrap of a list's frame
    numbers is the header's rule and not the fold of 2^31 and 2^31 + 1.  Negated -- M = 1, lens radius 0, the wrap taken as 2^31 -- the
    RIS, lens and wrap proofs fail (checked by hand when they were written)."""
import numpy as np
import pytest

import ao_oracle
import direct_oracle as do
import env_oracle
import extent_cases as xc
import extent_oracle as eo
import feature_oracle as fo
import lens_oracle
import moments_oracle as mom
import primary_accept
from conftest import assert_fb_equal
from env_scenes import env_scene
from oclpathtracer_amd.camera import Camera
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


# ---- the entry points added since: every proof is named after the corner its GPU cases name in their docstrings ----------------------
LATE_GIDS = np.arange(xc.LATE_W * xc.LATE_H)


def _late_ids(name):
    fb, n = xc.LATE[name]
    return np.tile(LATE_GIDS, n), np.repeat(np.arange(fb, fb + n, dtype=np.int64), len(LATE_GIDS))


def _corners(est):
    """(what, scene, W, H, gid, frame) of every TALL layout and LATE point an estimator is rendered at"""
    for name in xc.TALL:
        gid, frame = do.sample_ids(xc.TALL_W, xc.TALL_H, xc.LIT_FRAMES, **xc.TALL[name])
        yield "TALL " + name, xc.scene_of(est, True), xc.TALL_W, xc.TALL_H, gid, frame
    for name in xc.LATE:
        yield ("LATE " + name, xc.scene_of(est, False), xc.LATE_W, xc.LATE_H) + _late_ids(name)


def test_widened_feature_restatement_counts_pixels_as_the_walk_did():
    """feature_oracle.local_pixels is a closed form now (TALL has 2^25 - 1 rows): on every layout the suite uses and on every small one
    it is what the walk over the rows returned"""
    layouts = list(xc.EXISTING_LAYOUTS) + [(H, sr, nr, rank) for H in (1, 2, 5, 17, 40) for sr in (1, 2, 3, 6) for nr in (1, 2, 5)
                                           for rank in range(nr)]
    for H, sr, nr, rank in layouts:
        for W in (1, 3, 24):
            assert fo.local_pixels(W, H, sr, nr, rank) == sum(W for row in range(H) if (row // sr) % nr == rank), (W, H, sr, nr, rank)
    for name, s in xc.TALL.items():
        assert fo.local_pixels(xc.TALL_W, xc.TALL_H, **s) == xc.TALL_ROWS[name] * xc.TALL_W


@pytest.mark.parametrize("name", list(xc.TALL))
def test_tall_new_estimators_hit_and_miss(name):
    """TALL: the primary rays of the new estimators, of the features and of the lens AO render -- the pinhole's and the lens camera's,
    on TALL_SCENE -- hit the scene at some local pixels in every frame and miss it at others in every frame; no primary ray of the
    Cornell box misses on these layouts, which is why they are not rendered on it; the largest gid compared is the image's last"""
    for lens in (False, True):
        tri = xc.features_tall(name, lens).tri
        assert tri.shape == (xc.FEATURE_FRAMES, xc.TALL_ROWS[name] * xc.TALL_W)
        assert (tri >= 0).all(axis=0).any() and (tri < 0).all(axis=0).any(), "lens %d: %d hits, %d misses" % (lens, (tri >= 0).sum(), (tri < 0).sum())
        assert len(np.unique(tri[tri >= 0])) >= 3
    tris, mats = xc.cornell()[:2]
    closed = fo.samples(tris, mats, xc.TALL_W, xc.TALL_H, xc.FEATURE_FRAMES, **xc.TALL[name]).tri
    assert (closed >= 0).all(), "a primary ray leaves the Cornell box: the new cases could be rendered on it"
    gid = xc.tall_gids(name)
    assert gid.max() > 2 ** 31 - 2 ** 22 or name == "ragged"
    for est in xc.LIT_NEW:
        fb, rad = xc.lit_tall(est, name)
        assert np.isfinite(fb).all() and len(np.unique(rad.reshape(-1, 3), axis=0)) > 64, est
    assert max(xc.tall_gids(n).max() for n in xc.TALL) == xc.TALL_W * xc.TALL_H - 1 > 2 ** 31 - 2 ** 22


@pytest.mark.parametrize("est", ["ris_direct", "ris_indirect"])
def test_ris_keeps_a_later_candidate(est):
    """RIS: on each TALL layout and each LATE point some light sample keeps a candidate other than candidate 0 and some later candidate
    replaces a kept one -- with M = 1 neither can happen, and M = 8 would test nothing beyond it"""
    for what, sc, W, H, gid, frame in _corners(est):
        _, d = xc.lit_samples(est, sc, W, H, gid, frame, details=True)
        assert (d["kept"] > 0).any() and (d["replaced"] > 0).any(), "%s %s: candidate 0 is kept everywhere" % (est, what)
        assert d["kept"].max() < xc.LIT_M and (d["positive"] > 1).any()


@pytest.mark.parametrize("est", ["env_direct", "env_indirect"])
def test_env_samples_contribute(est):
    """Env: on each TALL layout and each LATE point an environment sample is open (it adds the map's light), and under env_indirect a
    BRDF ray leaves the scene and is weighted (wb != 1); the Cornell box, open towards the camera, does both, so it stays the scene"""
    for what, sc, W, H, gid, frame in _corners(est):
        _, d = xc.lit_samples(est, sc, W, H, gid, frame, details=True)
        assert (d["reason"] == env_oracle.R_OPEN).any(), "%s %s: no environment sample contributes" % (est, what)
        if xc.LIT[est].B is not None:
            left = d["miss_texel"] >= 0
            assert (left & (d["miss_wb"] != 1.0)).any(), "%s %s: no weighted ray leaves the scene" % (est, what)


def _lens_differs(W, H, gid, frame, tri_lens, tri_pin, what):
    cam = xc.lens_camera()
    o, d = lens_oracle.rays(cam, W, H, gid, frame)
    o0, d0 = lens_oracle.rays(cam, W, H, gid, frame, R=0.0, F=xc.LENS[1])
    assert (o != o0).any(axis=1).all(), "%s: %d lens rays start at the pinhole" % (what, int((~(o != o0).any(axis=1)).sum()))
    assert (o0 == np.asarray(cam.eye, np.float32)).all()
    assert (tri_lens != tri_pin).any(), "%s: every lens ray hits what the pinhole ray hits" % what


def test_lens_rays_are_not_the_pinholes():
    """Lens: on every TALL layout and at the LATE frames the lens rays differ from the pinhole rays of the same samples in origin at every
    sample, and the first-hit triangle differs for some -- otherwise the lens cases are the pinhole's"""
    for name in xc.TALL:
        gid, frame = do.sample_ids(xc.TALL_W, xc.TALL_H, xc.FEATURE_FRAMES, **xc.TALL[name])
        _lens_differs(xc.TALL_W, xc.TALL_H, gid, frame, xc.features_tall(name, True).tri, xc.features_tall(name, False).tri, name)
    gid, frame = _late_ids("last_frames")
    _lens_differs(xc.LATE_W, xc.LATE_H, gid, frame, xc.features_late(True).tri, xc.features_late(False).tri, "LATE last_frames")
    for name in ("table_end", "float_ties"):
        gid, frame = _late_ids(name)
        o, _ = lens_oracle.rays(xc.lens_camera(), xc.LATE_W, xc.LATE_H, gid, frame)
        assert (o != np.asarray(xc.lens_camera().eye, np.float32)).any(axis=1).all(), name
    rays = xc.lens_rays_late()
    assert rays.shape == (xc.LATE_W * xc.LATE_H, 8) and (rays[:, :3] != np.asarray(xc.lens_camera().eye, np.float32)).any(axis=1).all()
    cam = xc.lens_camera()
    pin = lens_oracle.camera_rays(Camera(cam.eye, cam.center), xc.LATE_W, xc.LATE_H, xc.LENS_RAYS_FRAME)
    assert (rays[:, 4:7] != pin[:, 4:7]).any(axis=1).all() and (pin[:, :3] == np.asarray(cam.eye, np.float32)).all()
    # the lens AO renders count something, and not what the pinhole counts
    for name in xc.TALL:
        c = xc.ao_lens_tall(name)
        assert 0 < c[..., 0].sum() < xc.AO_K * c[..., 1].sum() and (c[..., 1] == 0).any(), name
        pinhole = ao_oracle.counts(env_scene(xc.TALL_SCENE)[0], xc.TALL_W, xc.TALL_H, 0, 2, xc.AO_K, xc.AO_RADIUS, **xc.TALL[name])
        assert not np.array_equal(c, pinhole), name
    assert xc.ao_lens_late()[..., 1].sum() > 0


def test_features_late_and_tall_have_hits_and_misses():
    """Features: a hit and a miss per TALL layout (test_tall_new_estimators_hit_and_miss) and hits at the LATE frames; every output has
    values that differ between samples"""
    for lens in (False, True):
        s = xc.features_late(lens)
        assert s.tri.shape == (3, xc.LATE_W * xc.LATE_H) and (s.tri >= 0).any()
        for f in fo.FEATURES:
            assert len(np.unique(getattr(s, f).reshape(-1, 3), axis=0)) >= (2 if f == "emission" else 3), f   # (the panel emits or nothing does)
    for name in xc.TALL:
        s = xc.features_tall(name, False)
        assert (s.tri >= 0).any() and (s.tri < 0).any()
        assert (s.emission != 0).any() or name == "ragged", "%s: no sample sees the panel" % name


def test_fold_is_the_uniform_restatements():
    """xc.fold, which forms the list cases' framebuffers pixel by pixel, is the fold of the uniform restatements: resumed at the LATE
    points from late_start(), and from frame 0"""
    sc = xc.cornell()
    for name in xc.LATE:
        fb, n = xc.LATE[name]
        want, rad = xc.lit_late(xc.LIST_EST, name)
        assert_fb_equal(xc.fold_frames(xc.late_start(), rad, np.full(len(LATE_GIDS), fb)), want, name)
    rad = xc.lit_samples(xc.LIST_EST, sc, xc.LATE_W, xc.LATE_H, np.tile(LATE_GIDS, 3), np.repeat(np.arange(3), len(LATE_GIDS))).reshape(3, -1, 3)
    assert_fb_equal(xc.fold_frames(xc.late_start(), rad, np.zeros(len(LATE_GIDS))), xc.lit_render(xc.LIST_EST, sc, xc.LATE_W, xc.LATE_H, 0, 3), "0 .. 2")


@pytest.mark.parametrize("form", list(xc.LIST_FORMS))
def test_wrap_is_the_headers_rule(form):
    """Wrap: the uniform restatement of frames 2^31 - 2, 2^31 - 1, 0, 1 into late_start() equals that of frames 0, 1 into anything --
    frame 0 overwrites the pixel --, it is what the LATE list cases expect, and it differs from treating the wrapped numbers as 2^31
    and 2^31 + 1"""
    est, sc, W, H = xc.LIST_FORMS[form], xc.cornell(), xc.LATE_W, xc.LATE_H
    fb = xc.late_start()
    for first, n in ((2 ** 31 - 2, 1), (2 ** 31 - 1, 1), (0, 2)):
        fb = xc.lit_render(est, sc, W, H, first, n, start=fb)
    want = xc.lit_render(est, sc, W, H, 0, 2)
    assert_fb_equal(fb, want, "frames 2^31 - 2, 2^31 - 1, 0, 1 into late_start()")
    assert_fb_equal(xc.lit_render(est, sc, W, H, 0, 2, start=np.full((W * H, 4), 9.0, np.float32)), want, "frames 0, 1 into anything")
    first, frames = xc.LATE_LISTS["wrap"]
    ws, got, _ = xc.list_late(form, "wrap")
    assert xc.list_frames(first, frames)[:, 0].tolist() == [2 ** 31 - 2, 2 ** 31 - 1, 0, 1]
    assert_fb_equal(xc.fold_frames(xc.late_start(), ws, first), want, "the list case's expectation")
    assert_fb_equal(got, want, "the list case's expectation")
    unwrapped = xc.fold_frames(xc.late_start(), ws, first, wrap=False)
    assert (unwrapped[:, :3] != want[:, :3]).any(axis=1).sum() > len(want) // 2, "frame numbers 2^31 and 2^31 + 1 give the same pixels"
    # the mixed list: its even slots resume at 2046 across the reciprocal table's end, its odd slots wrap
    first, frames = xc.LATE_LISTS["mixed"]
    z = xc.list_frames(first, frames)
    assert z[:, 0].tolist() == [2046, 2047, 2048, 2049] and z[:, 1].tolist() == [2 ** 31 - 2, 2 ** 31 - 1, 0, 1] and set(first[:64:2]) != set(first[1:64:2])
    _, got, _ = xc.list_late(form, "mixed")
    resumed = xc.lit_render(est, sc, W, H, 2046, 4, start=xc.late_start())
    assert_fb_equal(got[0::2], resumed[0::2], "the slots at 2046")
    assert_fb_equal(got[1::2], want[1::2], "the slots that wrap")
    first, frames = xc.LATE_LISTS["float_ties"]
    assert_fb_equal(xc.list_late(form, "float_ties")[1], xc.lit_render(est, sc, W, H, int(first[0]), frames, start=xc.late_start()), "2^24 - 2")
    for case, offsets in xc.LATE_LIST_OFFSETS.items():
        assert min(xc.LATE_LISTS[case][0]) - max(offsets) >= 0


@pytest.mark.parametrize("form", list(xc.LIST_FORMS))
@pytest.mark.parametrize("name", xc.TALL_LIST_LAYOUTS)
def test_tall_lists_reach_the_last_pixel(form, name):
    """TALL lists: the list holds every third local pixel and the image's last, gid W * H - 1; the listed pixels hit and miss; the list
    render changes the listed pixels and records and nothing else"""
    px = xc.tall_list_pixels(name)
    gids = xc.tall_gids(name)
    assert gids[px].max() == xc.TALL_W * xc.TALL_H - 1 and len(px) == -(-len(gids) // 3) + (len(gids) % 3 != 1) and len(np.unique(px)) == len(px)
    tri = xc.features_tall(name, False).tri[:, px]
    assert (tri >= 0).any() and (tri < 0).any()
    fb0, rad0, m0, ws, fb1, m1 = xc.list_tall(form, name)
    assert ws.shape == (xc.TALL_LIST_FRAMES, len(px), 3) and len(np.unique(ws.reshape(-1, 3), axis=0)) > 64
    changed = (fb0 != fb1).any(axis=1)
    assert changed[px].sum() > len(px) // 2 and not np.delete(changed, px).any()
    rec0, rec1 = m0.view(mom.MOMENTS_DTYPE), m1.view(mom.MOMENTS_DTYPE)
    assert (rec1["n"][px] + rec1["rejected"][px] == 4).all() and (np.delete(rec1["n"] + rec1["rejected"], px) == 2).all()
    assert np.array_equal(np.delete(rec0, px), np.delete(rec1, px))
    # THE IDENTITY, for the form whose frames are all the uniform render's: four frames of it at the listed pixels
    if form == "pixels":
        four = xc.lit_render(xc.LIST_EST, xc.scene_of("ris_indirect", True), xc.TALL_W, xc.TALL_H, 0, 4, **xc.TALL[name])
        assert_fb_equal(fb1[px], four[px], "the uniform restatement after 4 frames")


def _far_samples(cols, frames):
    """how many samples of the WIDE row's columns ``cols`` over ``frames`` frames lie further from their pixel's centre ray than the
    mask kernel's eps: their jittered x, fl(x + r), is a neighbouring column's"""
    eps = float(_mask_eps())
    far = 0
    for x in cols:
        dc = _centre_dir(int(x), xc.WIDE_ROW)
        gid = xc.WIDE_ROW * xc.WIDE_W + int(x)
        for frame in range(frames):
            _, d, _ = ptoracle.generate_ray(int(x), xc.WIDE_ROW, xc.WIDE_W, xc.WIDE_H, gid + ptoracle.hash_u32(frame))
            far += float(np.abs(d.astype(np.float64) - dc).max()) > eps
    return far


def test_wide_list_reaches_the_window():
    """WIDE list: the listed window's columns lie at and above 2^23 and include hits of the box; over the 4 frames rendered some
    sample's jittered column fl(x + r) is an integer other than x (the WIDE proof's property); the sentinel columns are not listed"""
    cols = xc.wide_list_columns()
    window = xc.window_columns()
    assert np.isin(window, cols).all() and window.min() >= 2 ** 23 and len(cols) == 257 + 64 + 64 + xc.WIDE_LIST_SCATTERED
    assert cols[0] == 0 and cols[-1] == xc.WIDE_W - 1 and (np.diff(cols) > 0).all()
    guards = xc.wide_sentinel_columns()
    assert len(guards) == 8 and not np.isin(guards, cols).any()
    acc, _, _, _ = primary_accept.union(xc.cornell()[0], xc.WIDE_W, xc.WIDE_H, xc.WIDE_LIST_FRAMES, gid=xc.wide_gids(window))
    assert (primary_accept.popcount(acc) >= 1).sum() > 128, "the box covers few pixels of the window"
    assert _far_samples(window, xc.WIDE_LIST_FRAMES) > 0, "every sample of the window keeps its own column"
    ws, px = xc.wide_list()
    at = np.searchsorted(cols, window)
    assert len(np.unique(ws[:, at].reshape(-1, 3), axis=0)) > 64 and np.isfinite(px).all()


@pytest.mark.parametrize("est", list(xc.LIT))
def test_lit_tall_samples_carry_light(est):
    """the lit restatements take the TALL gids and late frames as they are, and their samples are not all background or black"""
    fb, rad = xc.lit_tall(est, "last_pixel")
    assert rad.shape == (xc.LIT_FRAMES, 512, 3) and fb.shape == (512, 4)
    assert len(np.unique(rad.reshape(-1, 3), axis=0)) > 64, "fewer than 65 different radiances in 1 024 samples"
    lfb, lrad = xc.lit_late(est, "last_frames")
    assert lrad.shape == (3, xc.LATE_W * xc.LATE_H, 3) and np.isfinite(lfb).all()
