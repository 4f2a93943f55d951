"""Every generated scene of the test suite, with the rays that query the LBVH's edge cases.  TEST INFRASTRUCTURE; everything is
generated from fixed seeds, and the order of the draws from a generator is part of each result.

  * building blocks: small, soup, soup_with_duplicates, nested_boxes;
  * scenes that steer the trace kernels and the LBVH builder: variant, bvh_edge, deep, horizon_tiles, random_quads;
  * scenes of up to 64 triangles, whose rays bring candidate masks: joined, box_prefix, sixty_four; sheets with sheet_rays, on which
    a ray's test accepts many triangles and the nearest is rarely the first (tests/masked_search_cases.py);
  * the far-origin scenes (tests/lbvh_far.py has their ray families): tile_scene, soup(2000, 5);
  * scenes at the edges of what the LBVH takes -- scale, offset, shape, the builder's boundaries -- with rays to query them:
    scene(name) for name in NAMES (tests/test_lbvh_scale_cpu.py: the oracle's scale identities; tests/test_gpu_lbvh_scenes.py);
  * slab: the boxes at unit scale beside ONE huge triangle that lifts the scene over PT_DET_BOUND_MAX -- the scene on which the
    unbounded kernels shade (tests/lit_cells.py), and as slab541 a cluster beside an outlier for the LBVH's builder;
  * scenes at the edges of direct illumination's light sample, each (tris, mats, lights, camera or None): direct_scaled,
    direct_light_list, direct_other_type, direct_from_behind (tests/test_direct_cpu.py proves that each reaches its edge,
    tests/test_gpu_direct_edges.py renders them); glossy_room, the GGX branch at every roughness a guard can meet (and, with
    FINITE_ROUGHNESS, at every one that keeps a multi-bounce path finite); edge_scene(name) names them all for the edge tests of
    direct and indirect illumination."""
from __future__ import annotations

import numpy as np

from oclpathtracer_amd import scene as _scene

SCALES = (-12, -11, -10, -9, 0, 20, 34, 40, 42, 43, 44, 45)   # 2^k; -9 .. 42: the oracle's hits are those of the unscaled scene
IDENTITY = tuple(k for k in SCALES if -9 <= k <= 42)          # outside: the literal det threshold / overflow thin the hits out
OFFSETS = (6, 10, 14)
RAYS = 16384


def small(rng, n, centres, size, nmat):
    """n triangles with p1 at the centres and p2, p3 within `size` of them on every axis; draws p2's offsets, p3's, the ids"""
    t = np.zeros(n, _scene.TRIANGLE_DTYPE)
    c = np.asarray(centres, np.float32)
    t["p1"][:, :3] = c
    t["p2"][:, :3] = c + rng.uniform(-size, size, (n, 3)).astype(np.float32)
    t["p3"][:, :3] = c + rng.uniform(-size, size, (n, 3)).astype(np.float32)
    t["id"] = rng.integers(0, nmat, n)
    return t


def _small_anywhere(rng, n, size=0.05):
    return small(rng, n, rng.uniform(-3, 3, (n, 3)), size, 7)


def soup(n=2000, seed=21, size=0.15):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, _scene.TRIANGLE_DTYPE)
    c = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = c + rng.normal(0, size, (n, 3)).astype(np.float32)
    t["id"] = rng.integers(0, 7, n)
    return t


def soup_with_duplicates(n, seed):
    t = soup(n, seed)
    t[n // 2: n // 2 + 40] = t[10:50]                        # duplicates: the lower index wins a tie
    return t


def nested_boxes(copies):
    """Nested, shrunk copies of the Cornell box: 8 copies are 288 triangles, 13 are 468 (the tiled brute-force kernel's range)"""
    tris, mats = _scene.load_model()
    parts = []
    for c in range(copies):
        t = tris.copy()
        k = np.float32(1.0 - 0.06 * c)
        for f in ("p1", "p2", "p3"):
            t[f][:, :3] = t[f][:, :3] * k + np.array([0.0, 2.7, -2.8], np.float32) * (np.float32(1.0) - k)
        parts.append(t)
    return np.concatenate(parts), mats


def variant(kind):
    """Scenes that steer the shim into each trace-kernel specialisation."""
    tris, mats = _scene.load_model()
    tris = tris.copy()
    if kind == "quads_scaled":      # still (2k, 2k+1) quads, other numbers: quad filter
        for f in ("p1", "p2", "p3"):
            tris[f][:, :3] = tris[f][:, :3] * np.float32(0.73) + np.array([0.11, 0.4, -0.2], np.float32)
    elif kind == "pairs_broken":    # same triangles, rotated by one: no pair is a quad: generic filter
        tris = np.roll(tris, 1)
    elif kind == "odd_count":       # 35 triangles
        tris = tris[:35].copy()
    elif kind == "huge_extent":     # |e1||e2| > 2e19: exact-division kernel (DET_BOUNDED = false)
        for f in ("p1", "p2", "p3"):
            tris[f][:, :3] = tris[f][:, :3] * np.float32(3.0e10)
    elif kind == "one_triangle":
        tris = tris[2:3].copy()
    elif kind == "degenerate":      # zero-area and NaN triangles among the real ones
        tris[4]["p2"] = tris[4]["p1"]
        tris[7]["p3"][:3] = np.nan
    elif kind == "quads_skewed":    # (a,b,c),(c,d,a) pairs far from parallelograms: shared-u filter, wide margins
        rng = np.random.default_rng(7)
        tris["p2"][1::2, :3] += rng.uniform(-0.4, 0.4, (len(tris) // 2, 3)).astype(np.float32)
    elif kind == "quads_tiny":      # the box shrunk to 5 cm in front of the eye: shared-u margins at their floor
        eye = np.array([0.0, 2.75, 4.0], np.float32)
        for f in ("p1", "p2", "p3"):
            tris[f][:, :3] = (tris[f][:, :3] - eye) * np.float32(0.01) + eye + np.array([0.0, 0.0, -0.05], np.float32)
    elif kind == "quads_detached":  # second triangles translated: e2' == -e2 still, p1' != p3: pair filter only
        for f in ("p1", "p2", "p3"):
            tris[f][1::2, :3] += np.array([0.25, -0.125, 0.5], np.float32)
    elif kind == "quads_nan_second":  # a NaN in the second triangle's e1 only: the pair structure survives
        tris["p2"][9, 1] = np.nan
    elif kind == "quads_17":        # an odd number of quads: the packed filter's last table entry is half padding
        tris = tris[:34].copy()
    elif kind == "quads_2":         # one pair of quads only
        tris = tris[4:8].copy()
    elif kind == "quads_72tri":     # three 32-triangle chunks: the box plus a shrunk copy of itself inside it
        inner = tris.copy()
        for f in ("p1", "p2", "p3"):
            inner[f][:, :3] = inner[f][:, :3] * np.float32(0.4) + np.array([0.3, 1.2, -1.9], np.float32)
        tris = np.concatenate([tris, inner])
    elif kind == "quads_far":       # scene far from the eye relative to its size: large radius, small triangles
        for f in ("p1", "p2", "p3"):
            tris[f][:, :3] = tris[f][:, :3] * np.float32(4.0) + np.array([0.0, -8.25, -160.0], np.float32)
    return tris, mats


def bvh_edge(kind):
    """Scenes that steer the LBVH builder into its corner cases (csrc/pt_bvh.hip: radix tree, eight-child collapse, big
    triangles outside the tree).  One generator serves every draw of a kind."""
    box, mats = _scene.load_model()
    rng = np.random.default_rng(99)
    some = lambda n, centres, size=0.05: small(rng, n, centres, size, len(mats))
    lo, span = np.array([-2.5, 0.2, -5.2]), np.array([5.0, 5.0, 5.0])
    if kind == "two":            # the smallest hierarchy: one node, two leaves
        return box[20:22].copy(), mats
    if kind == "three":
        return box[20:23].copy(), mats
    if kind == "nine":           # one more leaf than a node holds
        return some(9, lo + span * rng.random((9, 3)), 0.8), mats
    if kind == "duplicates":     # 300 copies of one triangle (equal Morton codes: the tree splits on the index bits) in the box
        t = some(1, (lo + span * 0.5)[None, :], 0.6)
        return np.concatenate([box, np.repeat(t, 300)]), mats
    if kind == "clustered":      # centres at 1 - 2^-k along the diagonal: every radix split peels one leaf off, a deep chain
        k = np.arange(1, 25)
        c = lo[None, :] + span[None, :] * (1.0 - 2.0 ** -k)[:, None]
        return np.concatenate([box, some(24, c, 0.02), some(400, lo + span * rng.random((400, 3)))]), mats
    if kind == "many_big":       # more big triangles than the brute-force table holds (64): they all stay in the tree
        return np.concatenate([box, some(90, lo + span * rng.random((90, 3)), 2.5), some(500, lo + span * rng.random((500, 3)))]), mats
    if kind == "flat":           # every centre in one plane: one Morton axis carries no information
        c = lo + span * rng.random((700, 3))
        c[:, 1] = 2.0
        return np.concatenate([box, some(700, c)]), mats
    raise ValueError(kind)


def deep():
    """A radix tree as deep as 30-bit Morton codes allow, then deeper through the index bits: nested clusters at 2^-k of the
    scene along the diagonal (k = 1 .. 10: every split peels one cluster off), each cluster a bundle of duplicates (equal
    Morton codes: the tree goes on splitting on the triangle index), inside a random soup that gives every ray work."""
    box, mats = _scene.load_model()
    rng = np.random.default_rng(5)
    lo, span = np.array([-2.5, 0.2, -5.2]), np.array([5.0, 5.0, 5.0])
    parts = [box]
    for k in range(1, 11):
        c = lo + span * (1.0 - 2.0 ** -k)
        one = small(rng, 1, c[None, :], 0.3 * 2.0 ** -k + 0.01, len(mats))
        parts.append(np.repeat(one, 40))                    # 40 copies: six more levels on the index bits
        parts.append(small(rng, 30, c[None, :] + rng.uniform(-1, 1, (30, 3)) * 2.0 ** -k, 0.02, len(mats)))
    parts.append(small(rng, 1500, lo + span * rng.random((1500, 3)), 0.06, len(mats)))
    return np.concatenate(parts), mats


def horizon_tiles(delta, tile=0.3, glossy_every=3):
    """Coplanar quads tiling the plane y = eye.y - delta, seen edge-on: the camera (GenerateColors.cl:265-276) looks along -z
    from (0, 2.75, 4), so the pixel rows just below the image centre meet this plane at cos(incidence) ~ delta / distance,
    from 1e-1 down to 1e-5 as delta shrinks, and every hit point lies next to the edges of several coplanar tiles -- where
    binary32's (u, v) of a grazing ray are least certain.  Tiles are smaller than 1/16 of the scene, so they all go INTO the
    hierarchy; neighbouring tiles have different materials (a wrong tile shows), every third one is glossy (its reflections
    leave 0.01 above the plane, GenerateColors.cl:257, and graze the next tiles)."""
    y = np.float32(2.75 - delta)
    xs = np.arange(-3.0, 3.0, tile, dtype=np.float32)
    zs = np.arange(-8.0, 3.95, tile, dtype=np.float32)
    nq = len(xs) * len(zs)
    tris = np.zeros(2 * nq, _scene.TRIANGLE_DTYPE)
    mats = np.zeros(8, _scene.MATERIAL_DTYPE)
    rng = np.random.default_rng(1)
    for m in range(8):
        mats[m]["albedo"] = tuple(rng.uniform(0.15, 0.95, 3)) + (1.0,)
        mats[m]["emissive"] = (30.0, 30.0, 30.0, 1.0) if m == 7 else (0.0, 0.0, 0.0, 1.0)
        mats[m]["type"] = _scene.SPECULAR if m % glossy_every == 0 else _scene.DIFFUSE
        mats[m]["roughness"] = np.float32(0.05) if m % glossy_every == 0 else 0.0
    q = 0
    s = np.float32(tile)
    for i, x in enumerate(xs):
        for j, z in enumerate(zs):
            a = np.array([x, y, z], np.float32)
            b = np.array([x, y, z + s], np.float32)
            c = np.array([x + s, y, z + s], np.float32)
            d = np.array([x + s, y, z], np.float32)
            # (a,b,c),(c,d,a) with cross(e2, e1) pointing DOWN: front-facing for rays that come from above (:100)
            for k, (p1, p2, p3) in enumerate(((a, b, c), (c, d, a))):
                t = tris[2 * q + k]
                t["p1"][:3], t["p2"][:3], t["p3"][:3] = p1, p2, p3
                t["id"] = (i * 5 + j * 3) % 8
            q += 1
    return tris, mats


def random_quads(seed: int):
    """Random (a,b,c),(c,d,a) quads around the view volume: parallelograms, perturbed parallelograms,
    slivers, huge and tiny ones, some facing away; random diffuse / glossy / emissive materials."""
    rng = np.random.default_rng(seed)
    nq = int(rng.integers(1, 40))
    tris = np.zeros(2 * nq, _scene.TRIANGLE_DTYPE)
    mats = np.zeros(nq, _scene.MATERIAL_DTYPE)
    scale = np.float32(10.0 ** rng.uniform(-1.5, 1.5))          # scene size: 0.03 ... 30
    centre = np.array([0.0, 2.75, 4.0], np.float32) + np.array([0.0, 0.0, -1.0], np.float32) * scale * np.float32(1.5)
    for q in range(nq):
        a = centre + rng.uniform(-1, 1, 3).astype(np.float32) * scale
        e1 = rng.uniform(-1, 1, 3).astype(np.float32) * scale * np.float32(10.0 ** rng.uniform(-1.5, 0.5))
        e2 = rng.uniform(-1, 1, 3).astype(np.float32) * scale * np.float32(10.0 ** rng.uniform(-1.5, 0.5))
        if rng.random() < 0.7 and np.dot(np.cross(e2, e1), a - np.array([0.0, 2.75, 4.0], np.float32)) < 0:
            e1, e2 = e2, e1                                      # most quads face the eye (cull test :100)
        b, c = a + e1, a + e1 + e2
        d = a + e2
        if rng.random() < 0.5:                                   # not a parallelogram
            d = d + rng.uniform(-0.3, 0.3, 3).astype(np.float32) * np.float32(np.abs(e1).max())
        for k, (p1, p2, p3) in enumerate(((a, b, c), (c, d, a))):
            t = tris[2 * q + k]
            t["p1"][:3], t["p2"][:3], t["p3"][:3] = p1, p2, p3
            t["id"] = q
        m = mats[q]
        m["albedo"] = tuple(rng.uniform(0.05, 0.95, 3)) + (1.0,)
        m["emissive"] = ((30.0, 30.0, 30.0, 1.0) if rng.random() < 0.15 else (0.0, 0.0, 0.0, 1.0))
        m["type"] = _scene.SPECULAR if rng.random() < 0.3 else _scene.DIFFUSE
        m["roughness"] = np.float32(10.0 ** rng.uniform(-2.5, -0.3)) if m["type"] == _scene.SPECULAR else 0.0
    return tris, mats


def joined(*parts):
    """scenes one after the other, the material indices of each moved behind the ones before"""
    tris, mats, base = [], [], 0
    for t, m in parts:
        t = t.copy()
        t["id"] += base
        base += len(m)
        tris.append(t)
        mats.append(m)
    return np.concatenate(tris), np.concatenate(mats)


def box_prefix(n):
    """the first n triangles of the Cornell box, with all its materials"""
    tris, mats = _scene.load_model()
    return tris[:n].copy(), mats


def sixty_four():
    """the box and two random quad scenes behind it: 64 triangles, both mask words full"""
    return joined(_scene.load_model(), random_quads(105), random_quads(1007))


SHEET_SPACING = 0.09375
SHEET_COPIES = ((5, 6), (1, 20), (25, 30))   # (quad, its copy): coincident triangles low/low, low/high and high/high in the mask words


def sheets(alternate=False, seed=20261021):
    """32 quads (a,b,c),(c,d,a) = 64 triangles parallel to z = const before the reference camera: half-sizes 1 .. 2.5, centres near
    (0, 2.75), stacked SHEET_SPACING apart from z = 1 downwards in an order that is a fixed shuffle of the quad index, all facing +z --
    a ray along -z passes the whole test of many triangles, and the nearest is rarely the lowest index.  Three whole quads are copies
    of others (SHEET_COPIES): their triangles tie in t, u and v bit for bit, and the lower index has to win.  alternate: the odd quads
    are mirrored to face -z, so that a bounced ray meets the sheets between."""
    rng = np.random.default_rng(seed)
    nq = 32
    level = rng.permutation(nq)
    tris = np.zeros(2 * nq, _scene.TRIANGLE_DTYPE)
    mats = np.zeros(nq, _scene.MATERIAL_DTYPE)
    for q in range(nq):
        hx, hy = (np.float32(h) for h in 1.0 + 1.5 * np.sqrt(rng.uniform(0.0, 1.0, 2)))   # (more large sheets than small ones)
        cx, cy = (np.float32(c) for c in np.array([0.0, 2.75]) + rng.uniform(-0.25, 0.25, 2))
        z = np.float32(1.0 - SHEET_SPACING * level[q])
        a, b, c, d = (cx - hx, cy - hy, z), (cx + hx, cy - hy, z), (cx + hx, cy + hy, z), (cx - hx, cy + hy, z)
        if alternate and q & 1:
            b, d = d, b
        for k, (p1, p2, p3) in enumerate(((a, b, c), (c, d, a))):
            t = tris[2 * q + k]
            t["p1"][:3], t["p2"][:3], t["p3"][:3] = p1, p2, p3
            t["id"] = q
        m = mats[q]
        m["albedo"] = tuple(rng.uniform(0.2, 0.95, 3)) + (1.0,)
        m["emissive"] = (12.0, 12.0, 12.0, 1.0) if q % 5 == 2 else (0.0, 0.0, 0.0, 1.0)
        m["type"] = _scene.SPECULAR if q % 7 == 3 else _scene.DIFFUSE
        m["roughness"] = np.float32(0.2) if m["type"] == _scene.SPECULAR else 0.0
    for src, dst in SHEET_COPIES:
        for f in ("p1", "p2", "p3"):
            tris[f][2 * dst: 2 * dst + 2] = tris[f][2 * src: 2 * src + 2]
    return tris, mats


def sheet_rays(n, seed=20261022):
    """pt_ray words for sheets(): 80 % of the origins before the stack and the rest inside it, directions about -z with a spread of
    0.35 and lengths 0.1 .. 10, a tenth of them turned the other way (everything is culled); the last eight rays hold a NaN or an
    infinity in the origin or the direction"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), np.float32)
    front = rng.uniform(size=n) < 0.8
    r[:, 0] = rng.uniform(-1.6, 1.6, n)
    r[:, 1] = 2.75 + rng.uniform(-1.6, 1.6, n)
    r[:, 2] = np.where(front, rng.uniform(1.05, 4.0, n), rng.uniform(1.0 - 31 * SHEET_SPACING, 1.0, n))
    r[:, 3] = 1e20
    d = np.concatenate([rng.normal(0.0, 0.35, (n, 2)), -np.ones((n, 1))], axis=1)
    d[rng.uniform(size=n) < 0.1] *= -1.0
    r[:, 4:7] = d * 10.0 ** rng.uniform(-1, 1, (n, 1))
    bad = np.array([np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf], np.float32)
    for k in range(8):
        r[n - 8 + k, (0, 1, 2, 4, 5, 6, 4, 2)[k]] = bad[k]
    return r


def tile_scene() -> np.ndarray:
    """A 24 x 24 checkerboard of axis-aligned quads (a,b,c),(c,d,a), cells of 0.25, in the plane y = 0.37 over [-3, 3]^2, every
    other cell left out: 288 quads = 576 triangles (512 or more: PT_OPT_ACCEL = 0 takes the LBVH too), normals +y."""
    y = np.float32(0.37)
    cells = [(i, j) for i in range(24) for j in range(24) if (i + j) % 2 == 0]
    t = np.zeros(2 * len(cells), _scene.TRIANGLE_DTYPE)
    for k, (i, j) in enumerate(cells):
        x0, x1, z0, z1 = -3 + 0.25 * i, -3 + 0.25 * (i + 1), -3 + 0.25 * j, -3 + 0.25 * (j + 1)
        a, b, c, d = (x0, y, z0), (x0, y, z1), (x1, y, z1), (x1, y, z0)
        t["p1"][2 * k, :3], t["p2"][2 * k, :3], t["p3"][2 * k, :3] = a, b, c
        t["p1"][2 * k + 1, :3], t["p2"][2 * k + 1, :3], t["p3"][2 * k + 1, :3] = c, d, a
        t["id"][2 * k: 2 * k + 2] = k % 7
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


def with_big(nbig, seed=31):
    """1 000 small triangles and exactly nbig whose longest box side is above 1/16 of the scene's (PT_BVH_BIG_MAX is 64)"""
    rng = np.random.default_rng(seed)
    big = _small_anywhere(rng, nbig, 0.05)
    big["p2"][:, 0] = big["p1"][:, 0] + np.float32(1.5)
    t = np.concatenate([_small_anywhere(rng, 1000), big])
    return t[rng.permutation(len(t))]


def non_finite(n, seed=41):
    rng = np.random.default_rng(seed)
    t = _small_anywhere(rng, n)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    t["p1"][np.arange(n), rng.integers(0, 3, n)] = bad[rng.integers(0, 3, n)]
    return t


def shared_point(n=600):
    """every vertex of every finite triangle is ONE point: the scene's extent is 0 on every axis; a few non-finite ones beside"""
    t = np.zeros(n, _scene.TRIANGLE_DTYPE)
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
    if name == "slab541":
        return edge_scene("slab:15")[1][0], slab_rays()
    raise ValueError(name)


NAMES = ["scale%d" % k for k in SCALES] + ["offset%d" % j for j in OFFSETS] + \
        ["squeezed", "stretched", "shared_point", "big64", "big65", "none_finite", "one_finite", "n511", "n512", "slab541"]


# ---- direct illumination: the light sample's edges ------------------------------------------------------------------------------
def direct_scaled(copies, k):
    """nested_boxes(copies) and the reference camera times 2^k (exact): the facing decisions stay, 0.01 and 0.02 do not scale, so
    at small k shadow rays have tl <= 0 and search nothing (at k = -9 all of them: the scene is smaller than 0.02)."""
    from oclpathtracer_amd.camera import Camera

    tris, mats = nested_boxes(copies)
    s = np.float32(2.0 ** k)
    for f in ("p1", "p2", "p3"):
        tris[f][:, :3] = tris[f][:, :3] * s
    ref = Camera.reference()
    cam = Camera(eye=tuple(np.float32(v) * s for v in ref.eye), center=tuple(np.float32(v) * s for v in ref.center), up=ref.up,
                 fov_y_deg=ref.fov_y_deg)
    return tris, mats, _scene.emitters(tris, mats), cam


SLAB_L, SLAB_L_BOUNDED = 2.5e9, 2.2e9
SLAB_P1 = (-60.0, -0.25, -2.5)
SLAB_EYE, SLAB_CENTER = (7.0, 4.5, 5.0), (0.0, 1.5, -2.5)


def slab_edges(L=SLAB_L):
    """(e1, e2) of the slab: diagonal in the plane y = const, so that |e1|_1 |e2|_1 = 4 L^2 while |e1 x e2| = 2 L^2"""
    return np.array([L, 0.0, L], np.float32), np.array([L, 0.0, -L], np.float32)


def slab(copies, L=SLAB_L, p1=SLAB_P1):
    """nested_boxes(copies) at unit scale plus ONE huge triangle, the last, 0.25 below the boxes' floor, with a material of its own (the
    last: a copy of material 0, diffuse, albedo 0.7), seen by an oblique camera.  The slab alone puts the scene above PT_DET_BOUND_MAX
    (4 L^2 = 2.5e19 > 2e19: L > 2.24e9), so every search of the scene is the unbounded one, while the camera, the boxes, the lights and
    the shadow rays are an ordinary scene's.  Its layout keeps the reference's triangle test precise: p1 lies near the scene (origin -
    p1 keeps the origin), the winding gives det > 0 for rays from above (one side is culled), and the normal's square 4 L^4 stays below
    FLT_MAX (L < 3.03e9), which axis-parallel edges of that L1 product cannot.  It covers the wedge x > -60, |z + 2.5| < x + 60.
    L = SLAB_L_BOUNDED is the bounded twin."""
    from oclpathtracer_amd.camera import Camera

    tris, mats = nested_boxes(copies)
    mats = np.concatenate([mats, mats[:1]])
    assert mats[-1]["type"] == _scene.DIFFUSE and abs(float(mats[-1]["albedo"][0]) - 0.7) < 1e-6 and not mats[-1]["emissive"][:3].any()
    one = np.zeros(1, _scene.TRIANGLE_DTYPE)
    e1, e2 = slab_edges(L)
    a = np.asarray(p1, np.float32)
    one["p1"][0, :3], one["p2"][0, :3], one["p3"][0, :3] = a, a + e1, a + e2
    one["id"] = len(mats) - 1
    tris = np.concatenate([tris, one])
    return tris, mats, _scene.emitters(tris, mats), Camera(eye=SLAB_EYE, center=SLAB_CENTER, up=(0.0, 1.0, 0.0), fov_y_deg=60.0)


SLAB_RAYS_W, SLAB_RAYS_H = 64, 32


def slab_rays(seed=541):
    """4 096 rays for slab(15), a cluster beside an outlier (the scene's extent is 5e9, the 540 small triangles share one cell of the
    LBVH's 16-bit grid, and the box margin PT_BVH_EPS x extent is wider than the cluster): the 64 x 32 primary rays of the scene's camera
    at frame 0 (the restatement of pt_camera_rays: they see the slab around the boxes), then 2 048 rays that start ON the slab, under
    the boxes and up to 2 beside them, and go upwards -- the slab culls them (they leave its back), the boxes' floor too, and what they
    hit is the inside of the boxes"""
    import query_oracle

    tris, _, _, cam = edge_scene("slab:15")[1]
    first = query_oracle.camera_rays(SLAB_RAYS_W, SLAB_RAYS_H, 0, cam)
    n = len(first)
    pts = np.concatenate([tris[f][:-1, :3] for f in ("p1", "p2", "p3")])
    lo, hi = pts.min(0) - np.float32(2.0), pts.max(0) + np.float32(2.0)
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, 0], r[:, 1], r[:, 2] = rng.uniform(lo[0], hi[0], n), SLAB_P1[1], rng.uniform(lo[2], hi[2], n)
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1])
    r[:, 3], r[:, 4:7] = 1e20, d
    return np.concatenate([first, r])


MIXED_SCALE = -7   # the k at which direct_scaled(10 or 15, k) has occluded, searched-open and unsearched shadow rays side by side

LIGHT_LIST = (36, 10, 10, 36, 3, 11)


def direct_light_list(lights=LIGHT_LIST):
    """The Cornell box plus triangle 36, a copy of light triangle 10 with p2 = p1 (no area: nj and cl are NaN); the default list is
    degenerate, duplicated, unsorted and holds a wall (3), which is sampled, casts its shadow ray and contributes 0."""
    tris, mats = _scene.load_model()
    extra = tris[10:11].copy()
    extra["p2"] = extra["p1"]
    tris = np.concatenate([tris, extra])
    assert len(tris) == 37
    return tris, mats, np.asarray(lights, np.int32), None


def direct_other_type():
    """The Cornell box with every diffuse material's type set to 3: neither branch of the BRDF (:220), all 3K uniforms drawn"""
    tris, mats = _scene.load_model()
    mats = mats.copy()
    diffuse = mats["type"] == _scene.DIFFUSE
    assert int(diffuse.sum()) == 8
    mats["type"][diffuse] = 3
    return tris, mats, _scene.emitters(tris, mats), None


BEHIND_EYE, BEHIND_CENTER = (0.0, 2.75, -10.0), (0.0, 2.75, -2.8)   # behind the back wall, looking at the box's middle


def direct_from_behind():
    """The Cornell box from outside: primary rays meet walls from their back, where the normal is negated (:243)"""
    from oclpathtracer_amd.camera import Camera

    tris, mats = _scene.load_model()
    return tris, mats, _scene.emitters(tris, mats), Camera(eye=BEHIND_EYE, center=BEHIND_CENTER, up=(0.0, 1.0, 0.0), fov_y_deg=60.0)


# Roughnesses of the glossy room, on both sides of every guard edge of the GGX branch that a roughness moves:
#   1 - xi over b = xi (r^2 - 1) + 1, b in [2^-60, 2^60):      b reaches r^2 for r > 1: r = 2^30;  for r < 2^-12, r^2 - 1 rounds
#                                                              to -1 and b is 1 - xi, +0 (xi = 1) included
#   r^2 / pi over gd^2, both in [2^-60, 2^60):                 r^2 / pi = 2^-60 at r = sqrt(pi) 2^-30, 2^60 at r = sqrt(pi) 2^30;
#                                                              gd^2 reaches r^4 for r > 1: r = 2^15 (and r^4 for 2^-12 < r < 1)
#   D cos / 4 dot(wo, wh) and D / 4 dwin dwon, D < 2^60:       D reaches 1 / (pi r^2): r = 2^-30 / sqrt(pi)
# and r = 1 (gd == 1 exactly), the Cornell box's own 0.008, the smallest r whose r^4 is a normal number, 0 (D = 0 / 0).
_SQRT_PI = float(np.sqrt(np.pi))
ROUGHNESS = [1.0, 0.008, float(np.nextafter(np.float32(2.0 ** -31.5), np.float32(1.0))), 0.0,
             2.0 ** 30 * 0.99, 2.0 ** 30 * 1.01,
             _SQRT_PI * 2.0 ** -30 * 0.99, _SQRT_PI * 2.0 ** -30 * 1.01, _SQRT_PI * 2.0 ** 30 * 0.99, _SQRT_PI * 2.0 ** 30 * 1.01,
             2.0 ** 15 * 0.99, 2.0 ** 15 * 1.01, 2.0 ** -12 * 0.99, 2.0 ** -12 * 1.01,
             2.0 ** -30 / _SQRT_PI * 0.99, 2.0 ** -30 / _SQRT_PI * 1.01, 0.3]


GLOSSY_SHIFTS = (0, 1, 4, 13)

# The roughnesses that keep a multi-bounce path finite.  The six others (indices 2, 3, 6, 7, 14, 15, all below 2e-9) turn every
# sample whose path bounces on them into NaN -- the BRDF sample's D is 0 / 0 or inf / inf there -- and a bit-exact comparison of a
# NaN sees nothing of the path after it (tests/test_indirect_cpu.py has the counts).
FINITE_ROUGHNESS = [ROUGHNESS[k] for k in (0, 1, 4, 5, 8, 9, 10, 11, 12, 13, 16)]


def glossy_room(shift=0, roughness=ROUGHNESS):
    """The Cornell box with every surface but the light a GGX one, a roughness of ``roughness`` each: the k-th such material takes
    roughness[(k + shift) % len(roughness)].  The reference camera sees seven of them lit by the light; GLOSSY_SHIFTS brings every
    one of ROUGHNESS onto one of those seven (direct illumination's GGX branch, tests/test_direct_cpu.py), FINITE_SHIFTS every one
    of FINITE_ROUGHNESS onto a surface that a path's later vertices meet lit (indirect illumination, tests/test_indirect_cpu.py)."""
    tris, mats = _scene.load_model()
    mats = mats.copy()
    k = 0
    for m in mats:
        if m["emissive"][0] != 0.0:
            continue
        m["type"] = _scene.SPECULAR
        m["roughness"] = np.float32(roughness[(k + shift) % len(roughness)])
        if m["albedo"][0] > 0.6:
            m["albedo"] = (0.5, 0.35, 0.05, 0.0)   # (a GGX weight is 2 albedo g dwin / pdf: keep long paths finite)
        k += 1
    assert k >= len(roughness)
    return tris, mats


# The smallest set of shifts that brings every FINITE_ROUGHNESS onto a surface where a path takes an OPEN light sample at a vertex
# i >= 1 (40 x 24, 3 frames, at K 1 / B 4 and at K 2 / B 6): no single shift of 0 .. 10 does, fifteen pairs do, and of those (5, 8)
# leaves its rarest roughness the most such samples (15; tests/test_indirect_cpu.py counts them again).
FINITE_SHIFTS = (5, 8)

_EDGE_SCENES = {}


def edge_scene(name):
    """(name, (tris, mats, lights or None, camera or None)) of a named input of the illumination edge tests, each built once:
    cornell, nested:COPIES, scaled:COPIES,K, slab:COPIES[,bounded], lights:list|36|10|all, glossy:SHIFT, finite:SHIFT, other_type, from_behind"""
    if name not in _EDGE_SCENES:
        kind, _, arg = name.partition(":")
        if kind == "cornell":
            sc = _scene.load_model() + (None, None)
        elif kind == "nested":
            sc = nested_boxes(int(arg)) + (None, None)
        elif kind == "scaled":
            copies, k = arg.split(",")
            sc = direct_scaled(int(copies), int(k))
        elif kind == "slab":   # slab:COPIES, or slab:COPIES,bounded for the twin below the bound
            copies, _, twin = arg.partition(",")
            sc = slab(int(copies), {"": SLAB_L, "bounded": SLAB_L_BOUNDED}[twin])
        elif kind == "lights":
            sc = direct_light_list(*{"list": (), "36": ([36],), "10": ([10],), "all": (np.arange(37),)}[arg])
        elif kind == "glossy":
            sc = glossy_room(int(arg)) + (None, None)
        elif kind == "finite":
            sc = glossy_room(int(arg), FINITE_ROUGHNESS) + (None, None)
        else:
            sc = {"other_type": direct_other_type, "from_behind": direct_from_behind}[kind]()
        _EDGE_SCENES[name] = sc
    return name, _EDGE_SCENES[name]
