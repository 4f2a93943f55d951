"""The numpy restatement of pt_sample_moments / pt_moments_resolve (tests/moments_oracle.py) against exact rational arithmetic, against
numpy's own variance and against the variance figure of tests/test_mis_cpu.py, without a GPU.  tests/test_gpu_moments.py compares the
device with this restatement bit for bit; here is why the restatement may be believed."""
from fractions import Fraction

import numpy as np

import mis_oracle as mo
import moments_oracle as mom
from scenes import edge_scene

RNG_SEED = 20


def _small_pixels(rng, pixels, frames, ratio):
    """float32 [frames, pixels, 3] with mean^2 / variance about ``ratio`` per pixel and channel (a normal distribution around a mean
    of sqrt(ratio) standard deviations), scales from 1e-3 to 1e3"""
    scale = (10.0 ** rng.uniform(-3, 3, (1, pixels, 3)))
    return ((rng.normal(size=(frames, pixels, 3)) + np.sqrt(ratio)) * scale).astype(np.float32)


def _exact(column):
    """(sum, sum of squares, unbiased variance) of a column of binary32 values, as Fractions"""
    xs = [Fraction(float(v)) for v in column]
    n = len(xs)
    s, q = sum(xs), sum(x * x for x in xs)
    return s, q, (q - s * s / n) / (n - 1)


def test_sums_are_the_correctly_rounded_sequential_sums():
    """Every step of the accumulation is one correctly rounded binary64 operation: sum' = round(sum + v), sum2' = round(sum2 + v v), with
    v v exact.  Checked per step in rational arithmetic (float(Fraction) rounds to nearest even) on 300 pixels of 17 frames."""
    rng = np.random.default_rng(RNG_SEED)
    s = _small_pixels(rng, 300, 17, 4.0)
    got = mom.accumulate(s)
    for p in range(300):
        for ch in range(3):
            run, run2 = 0.0, 0.0
            for f in range(17):
                v = Fraction(float(s[f, p, ch]))
                assert float(v * v) == float(s[f, p, ch]) ** 2 and Fraction(float(v * v)) == v * v     # the square is exact
                run, run2 = float(Fraction(run) + v), float(Fraction(run2) + v * v)
            assert got["sum"][p, ch] == run and got["sum2"][p, ch] == run2, (p, ch)
    assert (got["n"] == 17).all() and (got["rejected"] == 0).all()


def test_variance_against_exact_rational_arithmetic():
    """v within 1e-9 relative of the exact unbiased variance of the binary32 samples, on data with mean^2 / variance <= 100 and n <= 3 200.
    The two-sum form's error there is about n 2^-53 100 = 4e-11 relative (sum2 and sum mean are each about (1 + 100) n variance and
    carry n roundings of 2^-53 at the worst), so the bound has a factor of 25 over it."""
    rng = np.random.default_rng(RNG_SEED + 1)
    worst = 0.0
    for frames, pixels, ratio in ((3200, 8, 80.0), (3200, 8, 1.0), (257, 60, 50.0), (2, 100, 10.0), (31, 100, 0.0)):
        s = _small_pixels(rng, pixels, frames, ratio)
        mean, v = mom.resolve(mom.accumulate(s))
        for p in range(pixels):
            for ch in range(3):
                es, _, ev = _exact(s[:, p, ch])
                if frames > 2:   # (the bound is stated for mean^2 / variance <= 100: two samples can lie closer together than that)
                    assert (es / frames) ** 2 <= 100 * ev, "the data left the stated range"
                    err = abs(Fraction(float(v[p, ch])) - ev) / ev
                    worst = max(worst, float(err))
                    assert err <= Fraction(1, 10 ** 9), (frames, p, ch, float(err))
                assert abs(Fraction(float(mean[p, ch])) - es / frames) <= abs(es / frames) * Fraction(1, 10 ** 12)
    print("worst relative error of v against the exact variance: %.3g" % worst)


def test_variance_against_numpy():
    rng = np.random.default_rng(RNG_SEED + 2)
    s = _small_pixels(rng, 256, 640, 25.0)
    mean, v = mom.resolve(mom.accumulate(s))
    want = s.astype(np.float64).var(axis=0, ddof=1)
    assert np.allclose(v, want, rtol=1e-9, atol=0.0)
    assert np.allclose(mean, s.astype(np.float64).mean(axis=0), rtol=1e-12, atol=0.0)
    # the noise map is v rounded once; the summary's sums are the tree's, equal to a plain sum to rounding
    nm = mom.noise_map(mom.accumulate(s))
    assert np.array_equal(nm["var"], v.astype(np.float32)) and (nm["n"] == 640).all()
    sm = mom.summary(mom.accumulate(s))
    assert np.isclose(sm["var_sum"], v.sum(), rtol=1e-12) and np.isclose(sm["se2_sum"], (v / 640).sum(), rtol=1e-12)
    assert np.isclose(sm["mean2_sum"], (mean * mean).sum(), rtol=1e-12)
    assert int(sm["pixels"]) == 256 and int(sm["samples"]) == 256 * 640 and int(sm["rejected"]) == 0


def test_the_figure_of_test_mis_cpu_on_the_cornell_box():
    """tests/test_mis_cpu.py's _variance -- the population variance per pixel and channel over the frames, then the mean -- is
    variance_per_sample (n - 1) / n, to 1e-9, on the Cornell box at 16 x 16, 64 frames, K 1, B 4, plain and MIS."""
    from test_mis_cpu import _variance

    tris, mats = edge_scene("cornell")[1][:2]
    n = 64
    for mis in (False, True):
        rad = mo.radiance_frames(tris, mats, 16, 16, 0, n, 1, 4, mis=mis)
        assert np.isfinite(rad).all()
        fig = mom.noise(mom.accumulate(rad.astype(np.float32)))
        assert fig.pixels == 256 and fig.samples == 256 * n and fig.rejected == 0
        want = _variance(rad)
        print("mis %d: _variance %.9g, variance_per_sample (n - 1) / n %.9g" % (mis, want, fig.variance_per_sample * (n - 1) / n))
        assert abs(fig.variance_per_sample * (n - 1) / n - want) <= 1e-9 * want


def test_cancellation_resolves_to_plus_zero():
    """A pixel whose variance lies below n 2^-53 of its squared mean: sum2 - sum mean cancels.  A difference that comes out negative or
    zero resolves to +0 and one that comes out positive is a residue of that size -- never a negative variance, never -0, never NaN."""
    s = np.zeros((1000, 4, 3), np.float32)
    s[:, 0] = np.float32(0.1)                                     # constant, not a dyadic fraction: d is a rounding residue
    s[:, 1] = np.float32(1e19)                                    # constant and large: the squares reach 1e38 in binary64
    s[:, 2] = np.float32(3.0)
    s[::2, 3] = np.float32(1.0)
    s[1::2, 3] = np.nextafter(np.float32(1.0), np.float32(2.0))   # variance 2^-48 of the squared mean: below the threshold at n = 1000
    m = mom.accumulate(s)
    mean, v = mom.resolve(m)
    assert not np.isnan(v).any() and (v >= 0).all() and not np.signbit(v).any()
    assert v[2].tolist() == [0.0] * 3                             # exact sums of a small integer
    assert (v <= 4 * 1000 * 2.0 ** -53 * mean * mean).all()       # what is left is a rounding residue of the stated size
    d = m["sum2"] - m["sum"] * mean                               # the residues do take both signs, or the clamp would not be tested
    print("residues", d[:3].ravel())
    nm = mom.noise_map(m)
    assert not np.signbit(nm["var"]).any()
    assert mom.summary(m)["var_sum"] >= 0


def test_a_clamped_negative_residue_exists():
    """among constant pixels of many values some residue sum2 - sum mean is negative: the clamp is what keeps the variance at +0"""
    rng = np.random.default_rng(RNG_SEED + 3)
    s = np.repeat(rng.uniform(0.1, 10.0, (1, 500, 3)).astype(np.float32), 777, axis=0)
    m = mom.accumulate(s)
    mean, v = mom.resolve(m)
    d = m["sum2"] - m["sum"] * mean
    assert (d < 0).any() and (v[d <= 0] == 0).all() and (v >= 0).all() and not np.signbit(v).any() and not np.isnan(v).any()


def test_nonfinite_samples_are_rejected_and_leave_the_sums_alone():
    rng = np.random.default_rng(RNG_SEED + 4)
    s = _small_pixels(rng, 50, 40, 4.0)
    clean = mom.accumulate(s)
    bad = s.copy()
    where = rng.uniform(size=(40, 50)) < 0.2
    where[:, 7] = True                                            # a pixel with every sample rejected
    where[:, 8] = True
    where[11, 8] = False                                          # and one with exactly one finite sample
    ch = rng.integers(0, 3, (40, 50))
    val = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), (40, 50))
    f, p = np.nonzero(where)
    bad[f, p, ch[f, p]] = val[f, p]
    got = mom.accumulate(bad)
    kept = np.where(where[:, :, None], np.float32(0), s)          # the same samples with the rejected ones gone
    for px in range(50):
        want = mom.accumulate(kept[~where[:, px], px][:, None, :]) if (~where[:, px]).any() else mom.zeros(1)
        assert got["sum"][px].tobytes() == want["sum"][0].tobytes() and got["sum2"][px].tobytes() == want["sum2"][0].tobytes(), px
        assert got["n"][px] == (~where[:, px]).sum() and got["rejected"][px] == where[:, px].sum()
    assert got["n"][7] == 0 and got["rejected"][7] == 40 and got["n"][8] == 1
    mean, v = mom.resolve(got)
    assert (v[7] == 0).all() and (mean[7] == 0).all() and (v[8] == 0).all() and np.array_equal(mean[8], s[11, 8].astype(np.float64))
    sm = mom.summary(got)
    assert int(sm["samples"]) + int(sm["rejected"]) == 40 * 50 and int(sm["pixels"]) == int((got["n"] >= 2).sum()) <= 48
    assert clean["n"].sum() == 2000


def test_calls_merge_and_the_tree_is_fixed():
    rng = np.random.default_rng(RNG_SEED + 5)
    s = _small_pixels(rng, 33, 15, 4.0)
    whole = mom.accumulate(s)
    parts = mom.accumulate(s[6:], mom.accumulate(s[5:6], mom.accumulate(s[:5])))
    assert whole.tobytes() == parts.tobytes()
    x = rng.uniform(0, 1, 5)
    assert mom.tree_sum(x) == ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + 0.0) + (0.0 + 0.0))
    assert mom.tree_sum(x[:1]) == x[0] and mom.tree_sum(np.zeros(0)) == 0.0
    # padding further with +0 changes nothing (every contribution is >= +0): tiles of 2 048 and the next power of two agree
    y = rng.uniform(0, 1, 2049)
    padded = np.zeros(2048 * 2048)
    padded[:2049] = y
    assert mom.tree_sum(y) == mom.tree_sum(padded)
