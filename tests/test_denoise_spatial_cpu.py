"""pt_denoise_spatial without a device: its numpy restatement (tests/denoise_spatial_oracle.py) against pt_denoise's, the layout of its
parameter block, the argument errors the library reports before it needs a device, and what the pass is for -- on the Cornell box at
ONE sample a pixel pt_denoise returns the image as it found it, and the pooled variance lets the levels filter it.

``python tests/test_denoise_spatial_cpu.py`` prints the quality figures (profiles/denoise_spatial/quality.txt)."""
import ctypes
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import denoise_oracle as do
import denoise_spatial_oracle as dso
import moments_oracle as mo
from test_denoise_cpu import QB, QH, QK, QREF_BEGIN, QREF_FRAMES, QW, _guides

F = np.float32


def _mixed(rng, w, h):
    """records with n in 0 .. 4, scattered"""
    s = rng.uniform(0, 2, (4, w * h, 3)).astype(F)
    keep = rng.integers(0, 5, w * h)
    for f in range(4):
        s[f, keep <= f] = np.nan             # rejected: n = keep
    col = mo.accumulate(s)
    assert set(np.unique(col["n"])) == {0, 1, 2, 3, 4}
    return col


@pytest.mark.parametrize("below", [0, 1])
def test_below_0_and_1_are_pt_denoise(below):
    rng = np.random.default_rng(3)
    w, h = 11, 7
    col, gd = _mixed(rng, w, h), _guides(rng, w, h)
    for levels in (0, 2):
        for guides in (gd, [None] * 4):
            got = dso.denoise(col, *guides, w, h, below, levels=levels)
            assert got.tobytes() == do.denoise(col, *guides, w, h, levels=levels).tobytes()


def test_pool_touches_the_listed_pixels_alone():
    rng = np.random.default_rng(4)
    w, h = 11, 7
    col, gd = _mixed(rng, w, h), _guides(rng, w, h)
    base = do.denoise(col, *gd, w, h, levels=0)
    n = col["n"].reshape(h, w)
    for below in (2, 3, 5, 2 ** 31 - 1):
        got = dso.denoise(col, *gd, w, h, below, levels=0)
        pick = (n >= 1) & (n < below)
        assert np.array_equal(dso.listed(col, below).reshape(h, w), pick) and pick.any()
        assert np.array_equal(got[..., :3], base[..., :3]), "c changed"
        assert np.array_equal(got[~pick], base[~pick]), "a pixel that is not listed changed"
        assert np.isfinite(got).all() and (got[pick][:, 3] > 0).all()
        assert (got[pick][:, 3] != base[pick][:, 3]).any()


def test_box_pool_of_one_sample_pixels_by_hand():
    """no guide, every n = 1: the pool is the 7 x 7 box -- clipped at the border -- over the samples themselves, in binary64"""
    rng = np.random.default_rng(5)
    w, h = 6, 5
    s = rng.uniform(0, 2, (1, w * h, 3)).astype(F)
    col = mo.accumulate(s)
    got = dso.denoise(col, None, None, None, None, w, h, 2, levels=0)[..., 3]
    v = s[0].astype(np.float64).reshape(h, w, 3)
    for y in range(h):
        for x in range(w):
            wn, a, b = 0.0, np.zeros(3), np.zeros(3)
            for qy in range(max(0, y - 3), min(h, y + 4)):
                for qx in range(max(0, x - 3), min(w, x + 4)):
                    wn, a, b = wn + 1.0, a + v[qy, qx], b + v[qy, qx] * v[qy, qx]
            q = np.maximum(b / wn - (a / wn) * (a / wn), 0.0)
            assert got[y, x] == F((q[0] + q[1]) + q[2]), (x, y)


def test_params_block_and_errors_without_a_device():
    from oclpathtracer_amd import denoise, shim

    assert ctypes.sizeof(shim.DenoiseSpatialParams) == 32
    assert shim.DenoiseSpatialParams.below.offset == 0 and shim.DenoiseSpatialParams.reserved.offset == 4
    assert shim.PT_OPT_DENOISE_SPATIAL_FORM == 15
    lib = shim.load()
    p, sp = shim.DenoiseParams(), shim.DenoiseSpatialParams()
    none = [None] * 7
    assert lib.pt_denoise_spatial(None, *none, ctypes.byref(p), ctypes.byref(sp), None) == shim.PT_ERR_INVALID
    assert b"device" in lib.pt_last_error()
    assert lib.pt_denoise_spatial(None, *none, None, None, None) == shim.PT_ERR_INVALID
    assert lib.pt_device_set_option(None, shim.PT_OPT_DENOISE_SPATIAL_FORM, 1) == shim.PT_ERR_INVALID
    assert lib.pt_device_get_option(None, shim.PT_OPT_DENOISE_SPATIAL_FORM) == -1
    assert denoise.DEFAULTS == do.DEFAULTS and "spatial_below" not in denoise.DEFAULTS
    assert denoise.SPATIAL_BELOW == 2
    for bad in (-1, 1.5, 2 ** 31, True):
        with pytest.raises(ValueError):
            denoise.Denoiser(None, 4, 4, spatial_below=bad)


# ---- what the pass is for -------------------------------------------------------------------------------------------------------
_DATA = {}


def cornell_data(tris, mats):
    """(frame -> its one-sample records, the 256-frame reference [h, w, 3], frames -> guides), made once"""
    if not _DATA:
        import feature_oracle as fo
        import indirect_oracle as io

        def moments(begin, frames):
            m = None
            for f in range(begin, begin + frames, 32):   # (chunks: the sample arrays stay small)
                k = min(32, begin + frames - f)
                gid, frame = io.all_samples(QW, QH, k, f)
                m = mo.accumulate(io.samples(tris, mats, QW, QH, gid, frame, QK, QB)[0].reshape(k, QW * QH, 3), m)
            return m

        def guides(frames):
            fs = fo.samples(tris, mats, QW, QH, frames)
            return [mo.accumulate(getattr(fs, f)) for f in fo.FEATURES]

        _DATA.update(moments=moments, guides=guides, ref=mo.resolve(moments(QREF_BEGIN, QREF_FRAMES))[0].reshape(QH, QW, 3))
    return _DATA


def rel_mse(img, ref):
    """(mean, median) over the pixels of the relative MSE of profiles/denoise/quality.txt"""
    lum = ref.sum(axis=2)
    e = ((img[..., :3].astype(np.float64) - ref) ** 2).sum(axis=2) / (lum * lum / 3.0 + 0.01)
    return float(e.mean()), float(np.median(e))


def test_one_frame_is_filtered_with_the_pooled_variance(cornell):
    """Cornell 48 x 48, frame 0 alone against 256 frames from 1000.  pt_denoise returns the unfiltered image; below = 2 brings the
    median relative MSE below 0.5 of the unfiltered one (the prototype measured 0.18) and the mean below 1.0 (0.44)."""
    d = cornell_data(*cornell)
    col, gd, ref = d["moments"](0, 1), d["guides"](1), d["ref"]
    noisy = rel_mse(do.denoise(col, *gd, QW, QH, levels=0), ref)
    today = rel_mse(do.denoise(col, *gd, QW, QH), ref)
    pooled = rel_mse(dso.denoise(col, *gd, QW, QH, 2), ref)
    print("one frame: relative MSE mean / median unfiltered %.6g / %.6g, pt_denoise %.6g / %.6g, below = 2 %.6g / %.6g"
          % (noisy + today + pooled))
    assert abs(today[0] - noisy[0]) <= 1e-9 * noisy[0] and abs(today[1] - noisy[1]) <= 1e-9 * noisy[1], "pt_denoise filtered n = 1 pixels"
    assert pooled[1] < 0.5 * noisy[1]
    assert pooled[0] < 1.0 * noisy[0]


if __name__ == "__main__":
    from oclpathtracer_amd import scene

    d = cornell_data(*scene.load_model())
    ref = d["ref"]
    print("Cornell box %d x %d, B = %d, K = %d, uniform light choice, all four guides; reference: the mean of frames %d .. %d"
          % (QW, QH, QB, QK, QREF_BEGIN, QREF_BEGIN + QREF_FRAMES - 1))
    print("relative MSE per pixel: sum over channels of err^2 / (lum_ref^2 / 3 + 0.01), lum = r + g + b; mean / median over the pixels")
    print("defaults: %r" % (do.DEFAULTS,))
    print("%-34s %-22s %-22s %-22s %-22s" % ("input", "unfiltered", "pt_denoise (below = 0)", "below = 2", "below = 4"))
    fmt = lambda t: "%.4g / %.4g" % t
    for name, begin, frames in (("frame 0 alone", 0, 1), ("frame 100 alone", 100, 1), ("frames 0..1", 0, 2), ("frames 100..101", 100, 2),
                                ("frames 0..7", 0, 8)):
        col, gd = d["moments"](begin, frames), d["guides"](frames)
        row = [rel_mse(do.denoise(col, *gd, QW, QH, levels=0), ref), rel_mse(do.denoise(col, *gd, QW, QH), ref)]
        row += [rel_mse(dso.denoise(col, *gd, QW, QH, below), ref) for below in (2, 4)]
        print("%-34s %-22s %-22s %-22s %-22s" % ((name,) + tuple(fmt(t) for t in row)))
    # after a move: frames 0..7, but columns 20..25 hold frame 7 alone
    col, one, gd = d["moments"](0, 8), d["moments"](7, 1), d["guides"](8)
    x = np.arange(QW * QH) % QW
    short = (x >= 20) & (x <= 25)
    col[short] = one[short]
    sm = short.reshape(QH, QW)
    lum = ref.sum(axis=2)

    def split(img):
        e = ((img[..., :3].astype(np.float64) - ref) ** 2).sum(axis=2) / (lum * lum / 3.0 + 0.01)
        return (float(e[sm].mean()), float(np.median(e[sm]))), (float(e[~sm].mean()), float(np.median(e[~sm])))

    imgs = [do.denoise(col, *gd, QW, QH, levels=0), do.denoise(col, *gd, QW, QH)] + [dso.denoise(col, *gd, QW, QH, b) for b in (2, 4)]
    for k, name in ((0, "frames 0..7, cols 20..25 frame 7: those"), (1, "... the other pixels")):
        print("%-34s %-22s %-22s %-22s %-22s" % ((name[:34],) + tuple(fmt(split(i)[k]) for i in imgs)))
