"""The numpy restatement of pt_denoise_spatial (include/pt_shim.h states every step): pt_denoise's PREPARE and LEVELS are
denoise_oracle's, unchanged; POOL, between them, gives a pixel with 1 <= n < below the pooled per-sample variance of its guide-similar
7 x 7 neighbourhood.  The taps are shifted slices in the header's order -- dy outer, dx inner --, the weights binary32, the sums
binary64, every operation one numpy operation.  Nothing is compiled.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

import denoise_oracle as do

F = np.float32
D = np.float64
RADIUS = 3


def listed(colour, below):
    """the pixels POOL names: 1 <= n < below"""
    n = np.asarray(colour)["n"]
    return (n >= 1) & (n.astype(np.int64) < int(below))


def pool(colour, g, w, h, below, *, sigma_z, sigma_a, sigma_e, eps_z, normal_squarings, **_):
    """var [h, w] after POOL: g["var"] with the pooled variance at the listed pixels (g: denoise_oracle.prepare's planes)"""
    colour = np.asarray(colour)
    pick = listed(colour, below).reshape(h, w)
    if not pick.any():
        return g["var"]
    sigma_z, sigma_a, sigma_e, eps_z = (F(v) for v in (sigma_z, sigma_a, sigma_e, eps_z))
    cn = colour["n"].astype(D).reshape(h, w)
    cs, cs2 = colour["sum"].reshape(h, w, 3), colour["sum2"].reshape(h, w, 3)
    wn, a, b = np.zeros((h, w), D), np.zeros((h, w, 3), D), np.zeros((h, w, 3), D)
    with np.errstate(all="ignore"):
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                pq = do._slices(w, h, dx, dy)
                if pq is None:
                    continue
                p, q = pq
                if dx == 0 and dy == 0:
                    wt = np.ones((h, w), F)
                else:
                    x = np.zeros(cn[p].shape, F)
                    if g["z"] is not None:
                        t = (g["gx"][p] * F(dx)) + (g["gy"][p] * F(dy))
                        x = x + np.abs(g["z"][p] - g["z"][q]) / (sigma_z * np.abs(t) + eps_z)
                    if g["a"] is not None:
                        x = x + do._sq3(g["a"][p] - g["a"][q]) / sigma_a
                    if g["e"] is not None:
                        x = x + do._sq3(g["e"][p] - g["e"][q]) / sigma_e
                    y = F(1.0) + x * F(0.0625)
                    for _i in range(4):
                        y = y * y
                    wt = F(1.0) / y
                    if g["nrm"] is not None:
                        u, v = g["nrm"][p], g["nrm"][q]
                        d = ((u[..., 0] * v[..., 0]) + (u[..., 1] * v[..., 1])) + (u[..., 2] * v[..., 2])
                        d = np.where(d > 0, d, F(0.0))
                        for _i in range(int(normal_squarings)):
                            d = d * d
                        wt = wt * d
                assert wt.dtype == F
                wd = wt.astype(D)
                wn[p] = wn[p] + wd * cn[q]
                a[p] = a[p] + wd[..., None] * cs[q]
                b[p] = b[p] + wd[..., None] * cs2[q]
        m = a / wn[..., None]
        t = m * m
        v = b / wn[..., None] - t
        v = np.where(v > 0, v, 0.0)
        qk = v / cn[..., None]
        pooled = ((qk[..., 0] + qk[..., 1]) + qk[..., 2]).astype(F)
    return np.where(pick, pooled, g["var"])


def denoise(colour, albedo, normal, depth, emission, w, h, below, **params):
    """float32 [h, w, 4]: out of pt_denoise_spatial -- r, g, b, variance -- for moment records of w * h pixels (a guide may be None)"""
    kw = dict(do.DEFAULTS)
    kw.update(params)
    g = do.prepare(colour, albedo, normal, depth, emission, w, h)
    c, var = g["c"], pool(colour, g, w, h, below, **kw)
    for i in range(int(kw["levels"])):
        c, var = do.level(c, var, g, 1 << i, **kw)
    return np.concatenate([c, var[..., None]], axis=2).astype(F)
