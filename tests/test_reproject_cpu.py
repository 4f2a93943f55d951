"""pt_reproject without a device: properties of its numpy restatement (tests/reproject_oracle.py) on Cornell-box records from the CPU
oracles, the layout of its parameter block, the argument errors the library reports before it needs a device, and what the
reprojection is for -- after a camera move, history plus two new frames against two new frames alone.

``python tests/test_reproject_cpu.py`` prints the figures of profiles/reproject/quality.txt."""
import ctypes
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import moments_oracle as mo
import reproject_cases as rc
import reproject_oracle as ro

F = np.float32
W, H, FRAMES = 33, 17, 8
# the largest |fx - x|, |fy - y| of a covered pixel projected through its own camera at 33 x 17 (the reference camera and the panned
# one; profiles/reproject/quality.txt), and the bound the tests hold every projection to: 8 x that, the margin for other sizes' rounding
ROUND_TRIP = 3.82e-6   # (measured: 3.81e-6)
BOUND = 8 * ROUND_TRIP


def _case(cornell, prev, cur):
    """(history, previous features, current features) at 33 x 17: 8 frames under `prev`, one feature frame numbered on under `cur`
    (the previous features themselves when the cameras are the same)"""
    tris, mats = cornell
    col = rc.colour_records(tris, mats, W, H, prev, 0, FRAMES)
    pf = rc.feature_records(tris, mats, W, H, prev, FRAMES)
    cf = pf if cur == prev else rc.feature_records(tris, mats, W, H, cur, 1, FRAMES)
    return col, pf, cf


def _run(cornell, prev, cur, **kw):
    col, pf, cf = _case(cornell, prev, cur)
    cams = rc.cameras()
    return ro.reproject(col, pf["normal"], pf["depth"], cf["normal"], cf["depth"], W, H, cams[prev], cams[cur], **kw)


def round_trip(cornell):
    """max |fx - x| and |fy - y| over the covered pixels, a camera against itself, the larger of the reference and the panned camera"""
    worst = 0.0
    idx = np.arange(W * H)
    for name in ("ref", "panned"):
        _, pf, _ = _case(cornell, name, name)
        cams = rc.cameras()
        g = ro.project(pf["depth"], W, H, cams[name], cams[name])
        live = g["live"]
        assert live.sum() == (pf["depth"]["sum"][:, 1] > 0).sum() > 300          # every covered pixel comes back into the image
        worst = max(worst, float(np.abs(g["fx"][live] - (idx % W)[live]).max()), float(np.abs(g["fy"][live] - (idx // W)[live]).max()))
    return worst


@pytest.mark.parametrize("move", ["ref", "shifted", "panned"])
def test_two_identities(cornell, move):
    """max_history = 0 and a history of zero records write zero records, bit for bit"""
    out, info = _run(cornell, "ref", move, max_history=0)
    assert out.tobytes() == mo.zeros(W * H).tobytes() and not info[:, 3].any() and info[:, 2].any()
    col, pf, cf = _case(cornell, "ref", move)
    cams = rc.cameras()
    out, info = ro.reproject(mo.zeros(W * H), pf["normal"], pf["depth"], cf["normal"], cf["depth"], W, H, cams["ref"], cams[move])
    assert out.tobytes() == mo.zeros(W * H).tobytes() and not info[:, 2:].any()


def test_same_camera_round_trip(cornell):
    worst = round_trip(cornell)
    print("reproject round trip at %d x %d: max |fx - x|, |fy - y| = %.3g pixel" % (W, H, worst))
    assert 0 < worst <= BOUND
    tris, mats = cornell
    for name in ("ref", "panned"):
        col, pf, _ = _case(cornell, name, name)
        # away from depth and normal edges: every sample of the pixel and of its eight neighbours hit something, their mean normals
        # lie within 8 degrees of the pixel's and their mean depths within a quarter of it
        hit = (pf["tri"] >= 0).all(axis=0).reshape(H, W)
        nrm = mo.resolve(pf["normal"])[0].reshape(H, W, 3)
        z = (pf["depth"]["sum"][:, 0] / np.maximum(pf["depth"]["sum"][:, 1], 1.0)).reshape(H, W)
        same = np.zeros((H, W), bool)
        same[1:-1, 1:-1] = hit[1:-1, 1:-1]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                sl = (slice(1 + dy, H - 1 + dy), slice(1 + dx, W - 1 + dx))
                same[1:-1, 1:-1] &= hit[sl] & ((nrm[sl] * nrm[1:-1, 1:-1]).sum(axis=2) > 0.99) & (np.abs(z[sl] - z[1:-1, 1:-1]) < 0.25 * z[1:-1, 1:-1])
        inner = same.reshape(-1)
        assert inner.sum() > 50
        mean_prev = mo.resolve(col)[0]
        big = np.abs(mean_prev).reshape(H, W, 3)
        for cap in (3, 8, 100):
            out, info = _run(cornell, name, name, max_history=cap, max_noise=0.0)     # (the geometry alone: no record is set aside)
            want = np.minimum(col["n"], cap)
            assert ((out["n"] == want) | (out["n"] + 1 == want))[inner].all()
            assert (out["n"][inner] > 0).all() and (out["rejected"] == 0).all()
            assert (info[inner, 2] > 0.999).all()
            # the taps beside the pixel's own weigh tx + ty <= 2 BOUND together and each differs from it by at most twice the largest
            # |mean| of the 3 x 3 block: the merged mean lies within 4 BOUND of that (and a few binary64 roundings) of the old one
            block = np.zeros((H, W))
            block[1:-1, 1:-1] = np.max([big[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx].max(axis=2) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
            diff = np.abs(mo.resolve(out)[0] - mean_prev).max(axis=1)
            assert (diff[inner] <= (4 * BOUND + 1e-12) * block.reshape(-1)[inner]).all()


@pytest.mark.parametrize("move", ["shifted", "panned"])
def test_projection_against_binary64(cornell, move):
    """steps 2 and 3 restated independently in binary64 -- Camera.pinhole_ray and a plain perspective projection -- agree with the
    restatement's fx, fy within the round-trip bound"""
    _, pf, cf = _case(cornell, "ref", move)
    cams = rc.cameras()
    g = ro.project(cf["depth"], W, H, cams["ref"], cams[move])
    d = cams["ref"].derive().astype(np.float64)
    eye_p, view_p, hol_p, up_p, angle_p = d[0:3], d[3:6], d[6:9], d[9:12], d[12]
    s = cf["depth"]["sum"]
    checked = 0
    for p in np.nonzero(s[:, 1] > 0)[0]:
        x, y = p % W, p // W
        o, dirv = cams[move].pinhole_ray((x + 0.5) / W, (y + 0.5) / H, W / H)
        P = o + dirv * (s[p, 0] / s[p, 1])
        v = P - eye_p
        dz = v @ view_p
        if dz <= 0:
            assert not g["live"][p]
            continue
        fx = (v @ hol_p / dz / (angle_p * W / H) + 1.0) * 0.5 * W - 0.5
        fy = (1.0 - v @ up_p / dz / angle_p) * 0.5 * H - 0.5
        if -1 + BOUND < fx < W - BOUND and -1 + BOUND < fy < H - BOUND:
            assert g["live"][p]
            # (z itself is rounded to binary32 in the restatement: 2^-24 of a distance of at most 16, over a pixel of 0.07 at most)
            assert abs(fx - g["fx"][p]) <= BOUND and abs(fy - g["fy"][p]) <= BOUND, (p, fx, g["fx"][p], fy, g["fy"][p])
            checked += 1
    assert checked > 250


@pytest.mark.parametrize("move", ["ref", "shifted", "panned"])
def test_merged_variance_is_not_negative(cornell, move):
    """a weighted mean of second moments is at least the square of the weighted mean: sum2 - sum^2 / n >= 0 for every merged record, to
    the rounding of the dozen binary64 operations behind each side (2^-49 of sum2)"""
    out, _ = _run(cornell, "ref", move)
    took = out["n"] > 0
    assert took.sum() > 250
    n = out["n"][took].astype(np.float64)[:, None]
    d = out["sum2"][took] - out["sum"][took] * (out["sum"][took] / n)
    assert (d >= -(2.0 ** -49) * out["sum2"][took]).all()
    assert (mo.resolve(out)[1] >= 0).all()


DW = DH = 96


def disocclusion(cornell, **kw):
    """(pixels whose re-projected point is hidden from the old eye, those of them that took history, pixels re-projected) under the
    shifted camera at 96 x 96 -- the size at which the shift uncovers more than 50 pixels, so that 2 % is a pixel: hidden = the
    closest hit from the old eye towards P lies nearer than r (1 - 2 tol_z).  Every pixel of the history has 8 samples."""
    import query_oracle as qo

    tris, mats = cornell
    w, h = DW, DH
    cams = rc.cameras()
    tol_z = kw.get("tol_z", ro.DEFAULTS["tol_z"])
    col = mo.accumulate(np.ones((FRAMES, w * h, 3), F))
    pf = rc.feature_records(tris, mats, w, h, "ref", FRAMES)
    cf = rc.feature_records(tris, mats, w, h, "shifted", 1, FRAMES)
    g = ro.project(cf["depth"], w, h, cams["ref"], cams["shifted"])
    live = np.nonzero(g["live"])[0]
    eye = np.asarray(cams["ref"].eye, np.float64)
    v = g["P"][live].astype(np.float64) - eye
    rays = np.zeros((len(live), 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = eye, 1e20, v
    t = qo.closest(tris, rays)[:, 0].astype(np.float64)
    hidden = live[t < np.sqrt((v * v).sum(axis=1)) * (1.0 - 2.0 * tol_z)]
    out, _ = ro.reproject(col, pf["normal"], pf["depth"], cf["normal"], cf["depth"], w, h, cams["ref"], cams["shifted"], **kw)
    return len(hidden), int((out["n"][hidden] > 0).sum()), len(live)


def test_disoccluded_pixels_take_no_history(cornell):
    """at most 2 % of the hidden pixels may take history (silhouette pixels whose mean depth blends two surfaces are the allowance).
    The prototype measured 6 of 67 under min_weight = 0.25 -- a hidden point falls beside the silhouette, and the taps on its far side
    see the surface it lies on --, 2 under 0.5 and 1 under 0.6, which became the default: more than the nearest tap has to survive."""
    hidden, took, live = disocclusion(cornell)
    print("reproject disocclusion, shifted camera at %d x %d: %d of %d re-projected pixels are hidden from the old eye, %d of them took history"
          % (DW, DH, hidden, live, took))
    assert hidden >= 50, "the shift uncovers too little for 2 % to be a pixel"
    assert took <= 0.02 * hidden
    assert disocclusion(cornell, min_weight=0.0)[1] > took          # (the weight threshold is what keeps them out)


@pytest.mark.parametrize("move", ["shifted", "panned"])
def test_history_helps_after_a_move(cornell, move):
    """Figure (ii) -- history plus two new frames -- lies below figure (i) -- the two frames alone -- in relative MSE against 256
    frames under the new camera, in the mean and in the median.  Measured (profiles/reproject/quality.txt): mean 0.264 -> 0.198
    (shifted) and 0.242 -> 0.214 (panned), median 0.065 -> 0.015 for both; the mean is as good from 0.25 to 0.75.  WITHOUT the noise test (max_noise = 0) the mean does not
    hold, 2.56 and 2.02: five pixels of the 2 304 hold 98 % of the 8-frame history's own error (rare bright samples of the K = 1,
    uniform-choice estimator: its mean relative MSE against its own camera's reference is 5.97, its median 0.019), and whatever keeps
    the history's mean carries them over.  Those records have a squared standard error of 0.90 to 0.98 of their squared mean -- they
    know one sample --, 99 % of the records lie below 0.38; max_noise = 0.5 sets 0.6 % of the history aside."""
    tris, mats = cornell
    q = rc.quality(tris, mats, move)
    print("reproject quality, %s: relative MSE mean (i) %.6g (ii) %.6g (iii) %.6g; median (i) %.6g (ii) %.6g (iii) %.6g; share %.4f, mean length %.3f"
          % (move, q["alone"][1], q["merged"][1], q["perfect"][1], q["alone"][2], q["merged"][2], q["perfect"][2], q["share"], q["length"]))
    assert q["merged"][1] < q["alone"][1]
    assert q["merged"][2] < q["alone"][2]
    assert q["share"] > 0.8 and q["length"] == 8.0
    off = rc.quality(tris, mats, move, max_noise=0.0)
    assert off["share"] > q["share"] > off["share"] - 0.02          # (what the test sets aside is a small part of the history)


def test_noise_test_on_single_records():
    """one bright sample among seven dark ones: B equals the squared mean, so every max_noise in (0, 1) sets the record aside and 0
    keeps it; equal samples have B = 0 and always count; a record of one sample cannot be judged and counts"""
    w = h = 1
    dep = mo.accumulate(np.tile(np.array([[[5.5, 1.0, 1.0]]], F), (8, 1, 1)))       # the reference camera's centre ray, z = -1.5
    nrm = mo.accumulate(np.tile(np.array([[[0.0, 0.0, 1.0]]], F), (8, 1, 1)))
    spike = np.zeros((8, 1, 3), F)
    spike[3] = (40.0, 30.0, 20.0)
    flat = np.full((8, 1, 3), 0.5, F)
    run = lambda col, **kw: ro.reproject(mo.accumulate(col), nrm, dep, nrm, dep, w, h, None, None, **kw)[0]["n"][0]
    for mn in (0.01, 0.5, 0.99):
        assert run(spike, max_noise=mn) == 0 and run(flat, max_noise=mn) == 8 and run(spike[3:4], max_noise=mn) == 1
    assert run(spike, max_noise=0.0) == 8 and run(spike, max_noise=1.01) == 8
    mixed = flat.copy()
    mixed[3] = (2.0, 2.0, 2.0)                                                       # B / m^2 = 0.11
    assert run(mixed, max_noise=0.5) == 8 and run(mixed, max_noise=0.05) == 0


def test_params_block_and_errors_without_a_device():
    from oclpathtracer_amd import shim, temporal

    P = shim.ReprojectParams
    assert ctypes.sizeof(P) == 64
    assert (P.width.offset, P.height.offset, P.max_history.offset, P.tol_z.offset, P.cos_min.offset, P.min_weight.offset, P.max_noise.offset,
            P.reserved.offset) == (0, 4, 8, 12, 16, 20, 24, 28)
    lib = shim.load()
    sb = lib.pt_reproject_scratch_bytes
    assert sb(1, 1) > 0 and sb(1, 1) % 16 == 0 and sb(6, 4) == sb(4, 6) == sb(24, 1) == 24 * sb(1, 1)   # a function of width x height alone
    assert sb(0, 4) == 0 and sb(4, 0) == 0 and sb(-1, 4) == 0 and sb(4, -4) == 0
    assert sb(65536, 32768) == 0 and sb(46341, 46341) == 0                                               # above 2^31 - 1
    assert sb(0x7fffffff, 1) == 0x7fffffff * sb(1, 1)
    p = P()
    assert lib.pt_reproject(None, None, None, None, None, None, None, None, None, ctypes.byref(p), None, None, None) == shim.PT_ERR_INVALID
    assert b"device" in lib.pt_last_error()
    assert temporal.DEFAULTS == ro.DEFAULTS
    for bad in (dict(width=0), dict(height=0), dict(width=65536, height=32768), dict(max_history=-1), dict(max_history=1 << 31),
                dict(max_history=1.5), dict(tol_z=0.0), dict(tol_z=float("nan")), dict(tol_z=float("inf")), dict(tol_z=1e-50),
                dict(cos_min=-0.1), dict(cos_min=1.5), dict(cos_min=float("nan")), dict(min_weight=1.0), dict(min_weight=-0.5),
                dict(min_weight=float("nan")), dict(max_noise=-0.5), dict(max_noise=float("nan")), dict(max_noise=float("inf"))):
        kw = dict(width=4, height=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            temporal.Reprojector(None, kw.pop("width"), kw.pop("height"), **kw)


if __name__ == "__main__":
    from oclpathtracer_amd import scene

    cornell = scene.load_model()
    print("Cornell box %d x %d, B = 4, K = 1, uniform light choice.  History: frames 0 .. %d under the reference camera; one feature frame"
          % (rc.QW, rc.QH, rc.QHIST - 1))
    print("under the new camera; reference: the mean of frames %d .. %d under the new camera" % (rc.QREF_BEGIN, rc.QREF_BEGIN + rc.QREF_FRAMES - 1))
    print("relative MSE: sum over channels of err^2 / (lum_ref^2 / 3 + 0.01), lum = r + g + b; its mean and its median over the pixels")
    print("(i) frames 8 .. 9 under the new camera alone; (ii) the re-projected history plus those two; (iii) frames 8 .. 17 under the new camera")
    print("defaults: %r" % (ro.DEFAULTS,))
    for move, what in (("shifted", "eye and centre shifted by (0.3, 0, 0)"), ("panned", "a pan of 5 degrees about the up axis")):
        q = rc.quality(*cornell, move)
        print("%s:" % what)
        for key, name in (("alone", "(i)  "), ("merged", "(ii) "), ("perfect", "(iii)")):
            print("  %s MSE %.6g, relative MSE mean %.6g, median %.6g" % (name, q[key][0], q[key][1], q[key][2]))
        print("  covered pixels that took history: %.4f; mean history length: %.3f" % (q["share"], q["length"]))
        for mn in (0.0, 0.25, 0.75, 0.95):
            o = rc.quality(*cornell, move, max_noise=mn)
            print("  (ii) under max_noise = %.2f%s: MSE %.6g, relative MSE mean %.6g, median %.6g; took history %.4f"
                  % (mn, " (no noise test)" if mn == 0 else "", o["merged"][0], o["merged"][1], o["merged"][2], o["share"]))
    print("the means are firefly figures: of the 8-frame history's own relative MSE against its own camera's reference (mean 5.97, median")
    print("0.019) five pixels of 2 304 hold 98 %; frames 8 .. 9 happen to hold none, frames 10 .. 17 hold one far larger.  The noise test sets")
    print("a record aside whose mean's squared standard error exceeds max_noise of its squared mean: the five have 0.90 to 0.98 -- one bright")
    print("sample among dark ones has exactly 1 --, 99 % of the history's records lie below 0.38")
    hidden, took, live = disocclusion(cornell)
    print("disocclusion, shifted camera at %d x %d: %d of %d re-projected pixels are hidden from the old eye; %d of them took history" % (DW, DH, hidden, live, took))
    for mw in (0.0, 0.25, 0.5, 0.75):
        print("  under min_weight = %.2f: %d of %d" % ((mw,) + disocclusion(cornell, min_weight=mw)[1::-1]))
    print("round trip at %d x %d, a camera against itself: max |fx - x|, |fy - y| = %.3g pixel (the tests hold projections to 8 x %.3g)"
          % (W, H, round_trip(cornell), ROUND_TRIP))
