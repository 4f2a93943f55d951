"""Ray families and the margin measurement of the far-origin LBVH tests (tests/test_lbvh_margin_cpu.py on the host,
tests/test_gpu_lbvh_far.py on the device) over two scenes of tests/scenes.py.  TEST INFRASTRUCTURE; fixed seeds throughout.

The LBVH keeps, for every triangle, its box grown by eps = BVH_EPS x (the scene's largest |coordinate|).  That part of the margin
does not depend on the ray, while the displacement of a binary32 hit does: it grows with the distance the ray has travelled
(which is why the traversal adds a term sized by the ray's origin).  The families here aim at the EDGES of triangles -- where a
displaced hit leaves the triangle's box -- from D = (D/m) x m away, m the scene's largest |coordinate|.
"""
from __future__ import annotations

import numpy as np

from scenes import soup, tile_scene

BVH_EPS = 1.2e-4                       # PT_BVH_EPS (csrc/pt_bvh.hip)
DISTANCES = (1.0, 10.0, 100.0, 1e3, 1e4, 1e5)   # D / m
FAMILY_RAYS = 100_000
AIM = 4e-6                             # a ray is aimed within AIM x D / cos of an edge ...
TILE_CAP, SOUP_CAP = 0.125, 0.05       # ... but no farther than half a tile cell / a third of a soup triangle


SCENES = {"tile": (tile_scene, TILE_CAP), "soup": (lambda: soup(2000, 5), SOUP_CAP)}


def verts(tris) -> np.ndarray:
    """float64 [n, 3, 3]: the vertices as the device sees them (binary32 values)."""
    return np.stack([tris["p1"][:, :3], tris["p2"][:, :3], tris["p3"][:, :3]], 1).astype(np.float64)


def scene_m(tris) -> float:
    """the largest |coordinate| of the finite vertices, as pt_bvh_bounds_kernel takes it"""
    v = verts(tris)
    fin = np.isfinite(v).all((1, 2))
    return float(np.abs(v[fin]).max()) if fin.any() else 0.0


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _edge_targets(tris, rng, n, reach, cap):
    """n points within `reach` (per point, capped) of a random edge of a random triangle, in the triangle's plane, rounded to
    binary32; the unit normals e1 x e2 (the reference's test keeps rays that run AGAINST this normal, det > 0)."""
    v = verts(tris)
    k = rng.integers(0, len(v), n)
    e = rng.integers(0, 3, n)
    a, b = v[k, e], v[k, (e + 1) % 3]
    nrm = _unit(np.cross(v[k, 1] - v[k, 0], v[k, 2] - v[k, 0]))
    along = b - a
    perp = _unit(np.cross(nrm, along))
    off = rng.uniform(-1, 1, n) * np.minimum(reach, cap)
    tgt = a + rng.uniform(0, 1, (n, 1)) * along + off[:, None] * perp
    return tgt.astype(np.float32).astype(np.float64), nrm


def _pack(origin, direction, rng, tmax=1e20):
    """float32 [n, 8] pt_ray words; directions get lengths 1e-2 .. 1e2 (the device normalises as getRay does)"""
    n = len(origin)
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = origin
    r[:, 3] = tmax
    d = np.asarray(direction, np.float64) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    r[:, 4:7] = d.astype(np.float32)
    return r


def _tangent(nrm, rng):
    t = np.cross(nrm, rng.normal(size=nrm.shape))
    return _unit(t)


def family_edge(tris, cap, dm, rng, n=FAMILY_RAYS, cos_lo=0.01):
    """Rays from D = dm x m away at incidence cos in [cos_lo, 1) (log-uniform), aimed within AIM x D / cos of an edge, from the
    side the reference's test does not cull.  Returns (rays, cos)."""
    D = dm * scene_m(tris)
    cos = 10.0 ** rng.uniform(np.log10(cos_lo), 0.0, n)
    tgt, nrm = _edge_targets(tris, rng, n, AIM * D / cos, cap)
    u = -(cos[:, None] * nrm + np.sqrt(1 - cos * cos)[:, None] * _tangent(nrm, rng))   # the ray's direction
    o = (tgt - D * u).astype(np.float32)
    return _pack(o, tgt - o.astype(np.float64), rng), cos


def family_axis(tris, cap, dm, rng, n=FAMILY_RAYS):
    """Rays parallel to an axis (the other two components +-0), aimed at edges; four in five run along the axis on which the
    triangle's normal is longest, against the normal (the tile scene: -y), the others along a random signed axis."""
    D = dm * scene_m(tris)
    tgt, nrm = _edge_targets(tris, rng, n, np.full(n, AIM * D), cap)
    ax = np.abs(nrm).argmax(1)
    sg = -np.sign(nrm[np.arange(n), ax])
    rnd = rng.uniform(size=n) < 0.2
    ax = np.where(rnd, rng.integers(0, 3, n), ax)
    sg = np.where(rnd, np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0), sg)
    o = tgt.copy()
    o[np.arange(n), ax] -= sg * D
    d = np.zeros((n, 3))
    d[np.arange(n), ax] = sg
    r = _pack(o.astype(np.float32), d, rng)
    neg = (rng.uniform(size=(n, 3)) < 0.5) & (d == 0.0)
    r[:, 4:7][neg] = np.float32(-0.0)
    return r


def family_zero(tris, cap, dm, rng, n=FAMILY_RAYS):
    """Rays with ONE component +-0 (the ray stays in a coordinate plane through its target), otherwise as family_edge with
    cos >= 0.05 before the component is removed."""
    D = dm * scene_m(tris)
    cos = 10.0 ** rng.uniform(np.log10(0.05), 0.0, n)
    tgt, nrm = _edge_targets(tris, rng, n, AIM * D / cos, cap)
    u = -(cos[:, None] * nrm + np.sqrt(1 - cos * cos)[:, None] * _tangent(nrm, rng))
    z = np.abs(nrm).argsort(1)[np.arange(n), rng.integers(0, 2, n)]     # never the axis on which the normal is longest
    u[np.arange(n), z] = 0.0
    u = _unit(u)
    u *= np.where((u * nrm).sum(1) > 0, -1.0, 1.0)[:, None]             # still against the normal
    o = (tgt - D * u).astype(np.float32)
    d = tgt - o.astype(np.float64)
    assert np.all(d[np.arange(n), z] == 0.0)
    r = _pack(o, d, rng)
    neg = rng.uniform(size=n) < 0.5
    r[np.arange(n)[neg], 4 + z[neg]] = np.float32(-0.0)
    return r


def family_tmax(tris, cap, dm, rng, closest, n=FAMILY_RAYS):
    """Rays of family_edge (cos >= 0.03) that hit, with tmax EXACTLY the oracle's t (first half: that hit does not count, tmax
    is strict) and the next float above it (second half: it does).  closest: the oracle's search, rays -> [N, 12] records."""
    base, _ = family_edge(tris, cap, dm, rng, int(2.6 * n), cos_lo=0.03)
    w = closest(tris, base)
    hit = np.flatnonzero(w[:, 1].view(np.int32) >= 0)
    assert len(hit) >= n, "only %d of %d base rays hit" % (len(hit), len(base))
    r = base[hit[:n]].copy()
    t = w[hit[:n], 0]
    r[: n // 2, 3] = t[: n // 2]
    r[n // 2:, 3] = np.nextafter(t[n // 2:], np.float32(np.inf))
    return r


def families(name, dm, closest):
    """{family: rays} of scene `name` at distance dm x m: four families of FAMILY_RAYS rays each."""
    make, cap = SCENES[name]
    tris = make()
    seed = [ord(c) for c in name] + [int(np.log10(dm))]
    rng = lambda k: np.random.default_rng(seed + [k])
    return tris, {"edge": family_edge(tris, cap, dm, rng(0))[0], "axis": family_axis(tris, cap, dm, rng(1)),
                  "zero": family_zero(tris, cap, dm, rng(2)), "tmax": family_tmax(tris, cap, dm, rng(3), closest)}


def excess(tris, rays6, ray, tri):
    """How far outside its triangle's box an accepted hit really lies, per (ray, tri) record: the float64 crossing of the ray
    (binary32 origin, binary32 normalised direction: rays6 of query_oracle.get_rays) with the triangle's plane, and its largest
    distance beyond the box of the triangle's binary32 vertices over the three axes (0 inside).  In the scene's units."""
    v = verts(tris)[tri]
    o, d = rays6[ray, :3].astype(np.float64), rays6[ray, 3:].astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    s = ((v[:, 0] - o) * nrm).sum(1) / (d * nrm).sum(1)
    p = o + s[:, None] * d
    lo, hi = v.min(1), v.max(1)
    return np.maximum(np.maximum(lo - p, p - hi), 0.0).max(1)
