"""Scenes at the edges of what the LBVH takes -- scale, offset, shape, the builder's boundaries -- with rays to query them.
TEST INFRASTRUCTURE shared by tests/test_lbvh_scale_cpu.py (the oracle's scale identities) and tests/test_gpu_lbvh_scenes.py."""
from __future__ import annotations

import numpy as np

SCALES = (-12, -11, -10, -9, 0, 20, 34, 40, 42, 43, 44, 45)   # 2^k; -9 .. 42: the oracle's hits are those of the unscaled scene
IDENTITY = tuple(k for k in SCALES if -9 <= k <= 42)          # outside: the literal det threshold / overflow thin the hits out
OFFSETS = (6, 10, 14)
RAYS = 16384


def _dtype():
    from oclpathtracer_amd import scene

    return scene.TRIANGLE_DTYPE


def soup(n=2000, seed=21, size=0.15):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, _dtype())
    c = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = c + rng.normal(0, size, (n, 3)).astype(np.float32)
    t["id"] = rng.integers(0, 7, n)
    return t


def soup_rays(tris, n=RAYS, seed=22):
    """random rays through [-5, 5]^3, half of them aimed at triangle centroids"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-5, 5, (n, 3))
    r[:, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    k = rng.integers(0, len(tris), n // 2)
    cen = (tris["p1"][k, :3].astype(np.float64) + tris["p2"][k, :3] + tris["p3"][k, :3]) / 3
    r[: n // 2, 4:7] = cen - r[: n // 2, :3]
    return r


def transform(tris, rays, scale=(1.0, 1.0, 1.0), shift=0.0):
    """vertices and ray origins x scale + shift, rounded to binary32; directions x scale"""
    s = np.asarray(scale, np.float64)
    t, r = tris.copy(), rays.copy()
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = (tris[f][:, :3].astype(np.float64) * s + shift).astype(np.float32)
    r[:, :3] = (rays[:, :3].astype(np.float64) * s + shift).astype(np.float32)
    r[:, 4:7] = (rays[:, 4:7].astype(np.float64) * s).astype(np.float32)
    return t, r


def scaled(k):
    t = soup()
    r = soup_rays(t)
    s = 2.0 ** k
    t2, r2 = transform(t, r, (s, s, s))
    r2[:, 4:7] = r[:, 4:7]                      # (the directions stay: a uniform scale does not turn them)
    return t2, r2


def _small(rng, n, size=0.05):
    t = np.zeros(n, _dtype())
    c = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    t["p1"][:, :3] = c
    t["p2"][:, :3] = c + rng.uniform(-size, size, (n, 3)).astype(np.float32)
    t["p3"][:, :3] = c + rng.uniform(-size, size, (n, 3)).astype(np.float32)
    t["id"] = rng.integers(0, 7, n)
    return t


def with_big(nbig, seed=31):
    """1 000 small triangles and exactly nbig whose longest box side is above 1/16 of the scene's (PT_BVH_BIG_MAX is 64)"""
    rng = np.random.default_rng(seed)
    big = _small(rng, nbig, 0.05)
    big["p2"][:, 0] = big["p1"][:, 0] + np.float32(1.5)
    t = np.concatenate([_small(rng, 1000), big])
    return t[rng.permutation(len(t))]


def non_finite(n, seed=41):
    rng = np.random.default_rng(seed)
    t = _small(rng, n)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    t["p1"][np.arange(n), rng.integers(0, 3, n)] = bad[rng.integers(0, 3, n)]
    return t


def shared_point(n=600):
    """every vertex of every finite triangle is ONE point: the scene's extent is 0 on every axis; a few non-finite ones beside"""
    t = np.zeros(n, _dtype())
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = (1.0, 2.0, 3.0)
    t["p2"][::50, 1] = np.nan
    return t


def scene(name):
    """(triangles, rays) of a named case"""
    if name.startswith("scale"):
        return scaled(int(name[5:]))
    base = soup()
    rays = soup_rays(base)
    if name.startswith("offset"):
        return transform(base, rays, shift=2.0 ** int(name[6:]))
    if name == "squeezed":
        return transform(base, rays, (2.0 ** -20, 1.0, 1.0))
    if name == "stretched":
        return transform(base, rays, (1.0, 2.0 ** 20, 1.0))
    if name == "shared_point":
        r = rays.copy()
        r[: RAYS // 2, 4:7] = np.array([1.0, 2.0, 3.0], np.float32) - r[: RAYS // 2, :3]
        return shared_point(), r
    if name in ("big64", "big65"):
        t = with_big(int(name[3:]))
        return t, soup_rays(t)
    if name == "none_finite":
        return non_finite(5), rays
    if name == "one_finite":
        t = non_finite(601)
        t[300] = base[0]
        r = rays.copy()
        cen = (base["p1"][0, :3] + base["p2"][0, :3] + base["p3"][0, :3]) / np.float32(3)
        r[:, 4:7] = cen + np.random.default_rng(5).normal(0, 0.02, (RAYS, 3)).astype(np.float32) - r[:, :3]   # (one side is culled)
        return t, r
    if name in ("n511", "n512"):
        t = soup(int(name[1:]), 51, 0.3)
        return t, soup_rays(t)
    raise ValueError(name)


NAMES = ["scale%d" % k for k in SCALES] + ["offset%d" % j for j in OFFSETS] + \
        ["squeezed", "stretched", "shared_point", "big64", "big65", "none_finite", "one_finite", "n511", "n512"]
