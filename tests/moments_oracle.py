"""The numpy restatement of pt_sample_moments and pt_moments_resolve (include/pt_shim.h states every step): the accumulation is a loop
over the frames in ascending order, vectorised over the pixels in float64; resolve follows the header's operations one by one (numpy
rounds each on its own, and its float64 "/" is IEEE's); the summary's floating sums are the fixed tree, repeated x[0::2] + x[1::2]
on the array padded with +0 to a power of two.  Nothing is compiled.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import collections

import numpy as np

MOMENTS_DTYPE = np.dtype([("sum", np.float64, 3), ("sum2", np.float64, 3), ("n", np.uint32), ("rejected", np.uint32)])   # pt_pixel_moments
NOISE_DTYPE = np.dtype([("var", np.float32, 3), ("n", np.uint32)])                                                       # the noise record
SUMMARY_DTYPE = np.dtype([("var_sum", np.float64), ("se2_sum", np.float64), ("mean2_sum", np.float64),
                          ("pixels", np.uint64), ("samples", np.uint64), ("rejected", np.uint64)])                       # pt_noise_summary
assert MOMENTS_DTYPE.itemsize == 56 and NOISE_DTYPE.itemsize == 16 and SUMMARY_DTYPE.itemsize == 48

Noise = collections.namedtuple("Noise", "variance_per_sample relative_error pixels samples rejected")


def zeros(num_pixels: int) -> np.ndarray:
    return np.zeros(num_pixels, MOMENTS_DTYPE)


def accumulate(samples, moments=None) -> np.ndarray:
    """samples: [frames, pixels, 3] (binary32 values; a float64 array holding them is taken as it is); moments: the records to go on
    from (None: zeros, a reset).  A new array of records."""
    s = np.asarray(samples)
    assert s.ndim == 3 and s.shape[2] == 3, s.shape
    m = zeros(s.shape[1]) if moments is None else np.array(moments, MOMENTS_DTYPE)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(s.shape[0]):
            v = s[f].astype(np.float64)                   # (double)v: exact
            ok = np.isfinite(v).all(axis=1)
            add = np.where(ok[:, None], v, 0.0)
            sq = add * add                                # exact: the square of a converted binary32 value
            m["sum"][ok] = (m["sum"] + add)[ok]
            m["sum2"][ok] = (m["sum2"] + sq)[ok]
            m["n"] += ok.astype(np.uint32)                # uint32: wraps modulo 2^32
            m["rejected"] += (~ok).astype(np.uint32)
    return m


def resolve(moments):
    """(mean float64 [pixels, 3], v float64 [pixels, 3]) of the header's step 1"""
    m = np.asarray(moments)
    n = m["n"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mean = np.where(n > 0, m["sum"] / n, 0.0)
        t = m["sum"] * mean
        d = m["sum2"] - t
        v = d / (n - 1.0)
        v = np.where(v > 0, v, 0.0)
    v = np.where(n >= 2, v, 0.0)
    return mean, v


def noise_map(moments) -> np.ndarray:
    """the noise records: var = (float)v, rounded once, and n"""
    m = np.asarray(moments)
    out = np.zeros(len(m), NOISE_DTYPE)
    with np.errstate(over="ignore"):
        out["var"] = resolve(m)[1].astype(np.float32)
    out["n"] = m["n"]
    return out


def tree_sum(x) -> np.float64:
    """the fixed tree: padded with +0 to the next power of two, each level x'[i] = x[2 i] + x[2 i + 1]"""
    x = np.asarray(x, np.float64)
    size = 1
    while size < len(x):
        size *= 2
    p = np.zeros(size, np.float64)
    p[:len(x)] = x
    while len(p) > 1:
        p = p[0::2] + p[1::2]
    return p[0]


def summary(moments) -> np.ndarray:
    """the pt_noise_summary of the records, a SUMMARY_DTYPE scalar array"""
    m = np.asarray(moments)
    mean, v = resolve(m)
    n = m["n"].astype(np.float64)
    counted = m["n"] >= 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = (v[:, 0] + v[:, 1]) + v[:, 2]
        b = ((v[:, 0] / n) + (v[:, 1] / n)) + (v[:, 2] / n)
        c = ((mean[:, 0] * mean[:, 0]) + (mean[:, 1] * mean[:, 1])) + (mean[:, 2] * mean[:, 2])
    out = np.zeros((), SUMMARY_DTYPE)
    out["var_sum"] = tree_sum(np.where(counted, a, 0.0))
    out["se2_sum"] = tree_sum(np.where(counted, b, 0.0))
    out["mean2_sum"] = tree_sum(np.where(counted, c, 0.0))
    out["pixels"] = int(counted.sum())
    out["samples"] = int(m["n"].astype(np.uint64).sum())
    out["rejected"] = int(m["rejected"].astype(np.uint64).sum())
    return out


def noise(moments) -> Noise:
    """the figures DirectRenderer.noise() forms from the summary"""
    s = summary(moments)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_sample = float(s["var_sum"] / np.float64(3 * int(s["pixels"])))
        relative = float(np.sqrt(s["se2_sum"] / s["mean2_sum"]))
    return Noise(per_sample, relative, int(s["pixels"]), int(s["samples"]), int(s["rejected"]))
