"""The numpy restatement of pt_denoise (include/pt_shim.h states every step): binary32 arrays, every operation one numpy operation
(numpy rounds each on its own, its "/" and sqrt are IEEE's), the taps as shifted slices in the header's order -- dy outer, dx inner --,
so that every pixel's sums are taken in the order the contract states.  moments_oracle.resolve is step 1 of the variance.  Nothing is
compiled.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

import moments_oracle as mo

F = np.float32
DEFAULTS = dict(levels=5, sigma_l=4.0, sigma_z=1.0, sigma_a=0.01, sigma_e=0.01, eps_l=1e-6, eps_z=1e-4, normal_squarings=7)
KW = (F(0.375), F(0.25), F(0.0625))
KK = (F(0.5), F(0.25))


def _mean(m, w, h):
    """(float)(n > 0 ? sum / (double)n : 0), [h, w, 3]"""
    n = m["n"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(n > 0, m["sum"] / n, 0.0).astype(F).reshape(h, w, 3)


def prepare(colour, albedo, normal, depth, emission, w, h):
    """the prepared planes: dict of c [h, w, 3], var [h, w], and a, nrm, e [h, w, 3], z, gx, gy [h, w] (None for a guide left out)"""
    colour = np.asarray(colour)
    assert colour.shape == (w * h,), colour.shape
    g = {"c": _mean(colour, w, h)}
    _, v = mo.resolve(colour)
    n = colour["n"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        b = ((v[:, 0] / n) + (v[:, 1] / n)) + (v[:, 2] / n)
        g["var"] = np.where(colour["n"] >= 2, b, 0.0).astype(F).reshape(h, w)
    g["a"] = _mean(np.asarray(albedo), w, h) if albedo is not None else None
    g["nrm"] = _mean(np.asarray(normal), w, h) if normal is not None else None
    g["e"] = _mean(np.asarray(emission), w, h) if emission is not None else None
    g["z"] = g["gx"] = g["gy"] = None
    if depth is not None:
        s = np.asarray(depth)["sum"]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            z = np.where(s[:, 1] > 0, s[:, 0] / s[:, 1], 0.0).astype(F).reshape(h, w)
            xs, ys = np.arange(w), np.arange(h)
            g["gx"] = F(0.5) * (z[:, np.minimum(xs + 1, w - 1)] - z[:, np.maximum(xs - 1, 0)])
            g["gy"] = F(0.5) * (z[np.minimum(ys + 1, h - 1), :] - z[np.maximum(ys - 1, 0), :])
        g["z"] = z
    return g


def _slices(w, h, ox, oy):
    """(p, q) index pairs of the pixels whose tap at offset (ox, oy) lies inside the image; None when there are none"""
    x0, x1, y0, y1 = max(0, -ox), min(w, w - ox), max(0, -oy), min(h, h - oy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _sq3(d):
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def level(c, var, g, s, *, sigma_l, sigma_z, sigma_a, sigma_e, eps_l, eps_z, normal_squarings, want_sw=False, **_):
    """one a-trous level of step s: (c [h, w, 3], var [h, w]) -> the same; want_sw: the weight sums as a third result"""
    h, w = var.shape
    sigma_l, sigma_z, sigma_a, sigma_e, eps_l, eps_z = (F(v) for v in (sigma_l, sigma_z, sigma_a, sigma_e, eps_l, eps_z))
    with np.errstate(all="ignore"):
        lum = (c[..., 0] + c[..., 1]) + c[..., 2]
        gs, gk = np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                pq = _slices(w, h, dx, dy)
                if pq is None:
                    continue
                p, q = pq
                k = KK[abs(dx)] * KK[abs(dy)]
                gs[p] = gs[p] + k * var[q]
                gk[p] = gk[p] + k
        gv = gs / gk
        den_l = sigma_l * np.sqrt(gv) + eps_l
        sw, sv, sc = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pq = _slices(w, h, dx * s, dy * s)
                if pq is None:
                    continue
                p, q = pq
                hh = KW[abs(dx)] * KW[abs(dy)]
                if dx == 0 and dy == 0:
                    wt = np.full((h, w), hh, F)
                else:
                    x = np.zeros(var[p].shape, F)
                    if g["z"] is not None:
                        t = (g["gx"][p] * F(dx * s)) + (g["gy"][p] * F(dy * s))
                        x = x + np.abs(g["z"][p] - g["z"][q]) / (sigma_z * np.abs(t) + eps_z)
                    if g["a"] is not None:
                        x = x + _sq3(g["a"][p] - g["a"][q]) / sigma_a
                    if g["e"] is not None:
                        x = x + _sq3(g["e"][p] - g["e"][q]) / sigma_e
                    x = x + np.abs(lum[p] - lum[q]) / den_l[p]
                    y = F(1.0) + x * F(0.0625)
                    for _i in range(4):
                        y = y * y
                    wt = hh / y
                    if g["nrm"] is not None:
                        a, b = g["nrm"][p], g["nrm"][q]
                        d = ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])
                        d = np.where(d > 0, d, F(0.0))
                        for _i in range(int(normal_squarings)):
                            d = d * d
                        wt = wt * d
                assert wt.dtype == F
                sw[p] = sw[p] + wt
                sc[p] = sc[p] + wt[..., None] * c[q]
                sv[p] = sv[p] + (wt * wt) * var[q]
        out = sc / sw[..., None], sv / (sw * sw)
        assert out[0].dtype == F and out[1].dtype == F
    return out + (sw,) if want_sw else out


def denoise(colour, albedo, normal, depth, emission, w, h, **params):
    """float32 [h, w, 4]: out of pt_denoise -- r, g, b, variance -- for moment records of w * h pixels (a guide may be None)"""
    kw = dict(DEFAULTS)
    kw.update(params)
    g = prepare(colour, albedo, normal, depth, emission, w, h)
    c, var = g["c"], g["var"]
    for i in range(int(kw["levels"])):
        c, var = level(c, var, g, 1 << i, **kw)
    return np.concatenate([c, var[..., None]], axis=2).astype(F)
