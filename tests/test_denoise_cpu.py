"""pt_denoise without a device: properties of its numpy restatement (tests/denoise_oracle.py), the layout of its parameter block, the
argument errors the library reports before it needs a device, and what the filter is for -- on the Cornell box at 8 samples a pixel
the filtered image lies closer to a 256-frame reference than the unfiltered mean does.

``python tests/test_denoise_cpu.py`` prints the quality figures (profiles/denoise/quality.txt)."""
import ctypes
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import denoise_oracle as do
import moments_oracle as mo

F = np.float32


def _records(rng, w, h, frames=6, scale=1.0):
    """moments of `frames` random non-negative samples per pixel"""
    return mo.accumulate((rng.uniform(0, scale, (frames, w * h, 3))).astype(F))


def _guides(rng, w, h):
    """albedo, normal, depth, emission records of an image split into a left and a right surface"""
    left = (np.arange(w * h) % w) < (w + 1) // 2
    one = np.ones((4, w * h, 3), F)
    alb = one * np.where(left, 0.7, 0.2).astype(F)[None, :, None]
    nrm = one * np.where(left[:, None], (0, 0, 1), (1, 0, 0)).astype(F)[None]
    dep = one.copy()
    dep[..., 0] = np.where(left, 3.0, 5.0) + 0.01 * (np.arange(w * h) % w)
    dep[..., 2] = 0.5
    emi = np.zeros((4, w * h, 3), F)
    return [mo.accumulate(a) for a in (alb, nrm, dep, emi)]


def test_levels_0_is_the_prepared_image():
    rng = np.random.default_rng(1)
    w, h = 7, 5
    col = _records(rng, w, h)
    g = do.prepare(col, None, None, None, None, w, h)
    out = do.denoise(col, *_guides(rng, w, h), w, h, levels=0)
    assert out.dtype == F and out.shape == (h, w, 4)
    assert np.array_equal(out[..., :3], g["c"]) and np.array_equal(out[..., 3], g["var"])
    mean, v = mo.resolve(col)
    assert np.array_equal(g["c"].reshape(-1, 3), mean.astype(F))
    n = col["n"].astype(np.float64)
    assert np.array_equal(g["var"].reshape(-1), (((v[:, 0] / n) + (v[:, 1] / n)) + (v[:, 2] / n)).astype(F))
    assert (g["var"] > 0).all()


def test_prepare_edges_n0_n1_never_hit():
    w, h = 3, 2
    s = np.zeros((2, w * h, 3), F)
    s[:, 0] = np.nan                     # pixel 0: every sample rejected, n = 0
    s[1, 1] = np.inf                     # pixel 1: n = 1
    s[0, 1] = (1.0, 2.0, 3.0)
    s[0, 2:], s[1, 2:] = (0.5, 0.25, 0.125), (1.5, 0.75, 0.375)
    col = mo.accumulate(s)
    assert list(col["n"][:3]) == [0, 1, 2]
    dep = np.zeros((2, w * h, 3), F)     # pixel 4 is never hit: sum[1] = 0
    dep[..., 0], dep[..., 1] = 2.0, 1.0
    dep[:, 4] = 0.0
    g = do.prepare(col, None, None, mo.accumulate(dep), None, w, h)
    assert np.array_equal(g["c"][0, 0], (0, 0, 0)) and g["var"][0, 0] == 0
    assert np.array_equal(g["c"][0, 1], (1, 2, 3)) and g["var"][0, 1] == 0
    assert g["var"][0, 2] > 0
    assert g["z"][1, 1] == 0 and g["z"][0, 0] == 2
    # the gradient with clamped neighbours: pixel (0, 1) sees z(1, 1) = 0 on its right and itself on its left
    assert g["gx"][1, 0] == F(0.5) * (F(0) - F(2)) and g["gx"][0, 0] == 0 and g["gy"][0, 1] == F(0.5) * (F(0) - F(2))
    out = do.denoise(col, None, None, mo.accumulate(dep), None, w, h, levels=3)
    assert np.isfinite(out).all()


def test_centre_weight_keeps_the_sum_on_an_all_miss_image():
    """every guide zero, every colour zero, no variance: the taps' X are 0 / eps = 0 and w = h d with d = 0 (zero normals) -- only the
    centre tap, which no guide weighs, is left, and the output is 0 / (9 / 64), not 0 / 0"""
    w, h = 9, 6
    z = mo.accumulate(np.zeros((3, w * h, 3), F))
    g = do.prepare(z, z, z, z, z, w, h)
    c, var, sw = do.level(g["c"], g["var"], g, 1, want_sw=True, **do.DEFAULTS)
    assert np.array_equal(sw, np.full((h, w), F(9.0 / 64.0)))
    assert not c.any() and not var.any()
    # with live colours: under zero normals every other tap has weight 0 at every step; without the normal guide the others count
    rng = np.random.default_rng(5)
    col = _records(rng, w, h)
    for nrm in (z, None):
        g = do.prepare(col, z, nrm, z, z, w, h)
        for s in (1, 2, 4):
            _, _, sw = do.level(g["c"], g["var"], g, s, want_sw=True, **do.DEFAULTS)
            assert (sw >= F(9.0 / 64.0)).all() and ((sw == F(9.0 / 64.0)).all() if nrm is not None else (sw > F(9.0 / 64.0)).any())


@pytest.mark.parametrize("levels", [0, 1, 2, 5, 8])
def test_one_pixel_is_returned_unchanged(levels):
    rng = np.random.default_rng(levels)
    col = _records(rng, 1, 1)
    gd = _guides(rng, 1, 1)
    want = do.denoise(col, *gd, 1, 1, levels=0)
    got = do.denoise(col, *gd, 1, 1, levels=levels)
    # one tap, the centre's: c = (h c) / h and var = ((h h) var) / (h h) with h = 9/64.  9 x / 9 is x for most x, not for every x
    # (h h = 81/4096 is exact), so "unchanged" holds to the two roundings a level makes, 2^-24 each relative: what holds bit for
    # bit is the restatement of that one tap, and the image stays within levels * 2^-22 of the prepared one
    h = F(0.375) * F(0.375)
    c, var = want[0, 0, :3], want[0, 0, 3]
    for _ in range(levels):
        c, var = (h * c) / h, ((h * h) * var) / (h * h)
    assert np.array_equal(got[0, 0, :3], c) and got[0, 0, 3] == var
    assert np.allclose(got, want, rtol=levels * 2.0 ** -22, atol=0)


def test_smoothing_reduces_the_variance_and_respects_the_edge():
    rng = np.random.default_rng(11)
    w, h = 24, 10
    left = (np.arange(w * h) % w) < (w + 1) // 2
    s = rng.uniform(0.4, 0.6, (8, w * h, 3)).astype(F) * np.where(left, 1.0, 4.0).astype(F)[None, :, None]
    col = mo.accumulate(s)
    gd = _guides(rng, w, h)
    out = do.denoise(col, *gd, w, h)
    pre = do.denoise(col, *gd, w, h, levels=0)
    # (inside a region every tap is alike, so the first level alone leaves (sum of kw^2)^2 = 0.075 of the variance; the pixels at
    # the edge and the border keep more: a fifth over the image is far above that)
    assert out[..., 3].mean() < 0.2 * pre[..., 3].mean()
    lum = out[..., :3].sum(axis=2).reshape(-1)
    assert abs(lum[left].mean() - 1.5) < 0.05 and abs(lum[~left].mean() - 6.0) < 0.2   # no bleeding across the albedo / normal edge
    # without any guide the luminance term alone must hold that edge apart less well or as well, never produce a non-finite value
    assert np.isfinite(do.denoise(col, None, None, None, None, w, h)).all()


def test_params_block_and_errors_without_a_device():
    from oclpathtracer_amd import shim

    assert ctypes.sizeof(shim.DenoiseParams) == 64
    assert shim.DenoiseParams.sigma_l.offset == 16 and shim.DenoiseParams.eps_l.offset == 32 and shim.DenoiseParams.reserved.offset == 40
    lib = shim.load()
    sb = lib.pt_denoise_scratch_bytes
    assert sb(1, 1) > 0 and sb(6, 4) == sb(4, 6) == sb(24, 1) == 24 * sb(1, 1)          # a function of width x height alone
    assert sb(0, 4) == 0 and sb(4, 0) == 0 and sb(-1, 4) == 0 and sb(4, -4) == 0
    assert sb(65536, 32768) == 0 and sb(46341, 46341) == 0                               # above 2^31 - 1
    assert sb(0x7fffffff, 1) == 0x7fffffff * sb(1, 1) and sb(46340, 46341) == 46340 * 46341 * sb(1, 1)
    p = shim.DenoiseParams()
    assert lib.pt_denoise(None, None, None, None, None, None, None, None, ctypes.byref(p), None) == shim.PT_ERR_INVALID
    assert b"device" in lib.pt_last_error()
    from oclpathtracer_amd import denoise

    assert denoise.DEFAULTS == do.DEFAULTS
    for bad in (dict(width=0), dict(height=0), dict(width=65536, height=32768), dict(levels=9), dict(levels=-1), dict(normal_squarings=9),
                dict(sigma_l=0.0), dict(sigma_a=float("nan")), dict(eps_z=float("inf")), dict(eps_l=1e-50), dict(sigma_z=-1.0)):
        kw = dict(width=4, height=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            denoise.Denoiser(None, kw.pop("width"), kw.pop("height"), **kw)


# ---- what the filter is for ----------------------------------------------------------------------------------------------------
QW = QH = 48
QFRAMES, QREF_BEGIN, QREF_FRAMES, QB, QK = 8, 1000, 256, 4, 1


def quality(tris, mats, without=(), **params):
    """(MSE ratio, relative-MSE ratio, the four figures) of the filtered against the unfiltered 8-frame mean of the Cornell box at
    48 x 48, B = 4, K = 1, the uniform light choice, both against the mean of frames 1000 .. 1255; without: the guides left out"""
    import feature_oracle as fo
    import indirect_oracle as io

    def moments(begin, frames):
        m = None
        for f in range(begin, begin + frames, 32):   # (chunks: the sample arrays stay small)
            k = min(32, begin + frames - f)
            gid, frame = io.all_samples(QW, QH, k, f)
            m = mo.accumulate(io.samples(tris, mats, QW, QH, gid, frame, QK, QB)[0].reshape(k, QW * QH, 3), m)
        return m

    col = moments(0, QFRAMES)
    ref = mo.resolve(moments(QREF_BEGIN, QREF_FRAMES))[0].reshape(QH, QW, 3)
    fs = fo.samples(tris, mats, QW, QH, QFRAMES)
    guides = [mo.accumulate(getattr(fs, f)) if f not in without else None for f in fo.FEATURES]
    noisy = do.denoise(col, *guides, QW, QH, levels=0)[..., :3].astype(np.float64)
    filt = do.denoise(col, *guides, QW, QH, **params)[..., :3].astype(np.float64)
    lum = ref.sum(axis=2)
    den = lum * lum / 3.0 + 0.01

    def figures(img):
        e2 = ((img - ref) ** 2).sum(axis=2)
        return float(e2.mean()), float((e2 / den).mean())

    (mse0, rel0), (mse1, rel1) = figures(noisy), figures(filt)
    return mse1 / mse0, rel1 / rel0, (mse0, rel0, mse1, rel1)


def test_filtered_image_is_closer_to_the_reference(cornell):
    """Cornell 48 x 48, 8 frames against 256 frames from 1000.  The prototype measured an MSE ratio of 0.395 and a relative-MSE ratio
    of 0.025 under the defaults; the bound of 0.1 leaves room for a justified retuning of the defaults only."""
    tris, mats = cornell
    mse_ratio, rel_ratio, figs = quality(tris, mats)
    print("denoise quality: MSE %.6g -> %.6g (ratio %.4f), relative MSE %.6g -> %.6g (ratio %.4f)"
          % (figs[0], figs[2], mse_ratio, figs[1], figs[3], rel_ratio))
    assert mse_ratio < 1.0, "the filter makes the image worse"
    assert rel_ratio < 0.1


if __name__ == "__main__":
    from oclpathtracer_amd import scene

    t, m = scene.load_model()
    fo_all = ("albedo", "normal", "depth", "emission")
    print("Cornell box %d x %d, %d frames, B = %d, K = %d, uniform light choice; reference: the mean of frames %d .. %d"
          % (QW, QH, QFRAMES, QB, QK, QREF_BEGIN, QREF_BEGIN + QREF_FRAMES - 1))
    print("relative MSE: sum over channels of err^2 / (lum_ref^2 / 3 + 0.01), lum = r + g + b, averaged over the pixels")
    print("defaults: %r" % (do.DEFAULTS,))
    for name, kw in (("all four guides", {}), ("no emission guide", dict(without=("emission",))), ("no guide at all", dict(without=fo_all))):
        a, b, figs = quality(t, m, **kw)
        print("%s:\n  MSE %.6g -> %.6g, ratio %.4f\n  relative MSE %.6g -> %.6g, ratio %.4f" % (name, figs[0], figs[2], a, figs[1], figs[3], b))
