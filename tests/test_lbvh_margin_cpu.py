"""The LBVH's documented margin, measured with the CPU oracle alone (no GPU).

The hierarchy keeps every triangle's box grown by eps = PT_BVH_EPS x m (m: the scene's largest |coordinate|), and the traversal
widens every slab by w = PT_BVH_RAY_EPS x (the ray origin's largest |coordinate|).  A hit that binary32's triangle test accepts is
lost if the exact ray passes the triangle's box farther out than that.  The quantity here is that distance -- the EXCESS: how far
the float64 crossing of the ray (binary32 origin, direction normalised in binary32 as getRay does) with the triangle's plane lies
outside the box of the accepted triangle's binary32 vertices -- over 400 000 rays aimed at triangle edges at incidence
cos 0.01 .. 1 from D = (D/m) x m away (tests/lbvh_far.py), for EVERY triangle the exact test accepts for a ray
(query_oracle.all_hits), on a 576-triangle checkerboard in one plane and on a 2 000-triangle soup.

MEASURED holds what the reference's arithmetic gave on these inputs; the asserted bounds are twice that (the spread of a maximum
over 4 x 10^5 rays from seed to seed), and every measured share of the margin eps + w must itself be at most 0.5: half the margin
is spare.  SCENE_ONLY holds the same excess in units of eps alone, the margin the hierarchy had before the ray term: on the
checkerboard it stays at 0.10 eps up to D/m = 100, as documented; on the soup ONE accepted hit of 372 805 at D/m = 100 (incidence
cos 0.0123) lies 1.07 eps outside its box -- more than the 0.5 that margin was meant to keep -- and from D/m = 1000 on hundreds
do.  That is why the near distances, too, are held against eps + w here, and why the scene margin alone at D/m = 100 is only
bounded by what was measured (no claim that it suffices there).  Up to D/m = 10 it does on both scenes (0.0052 eps, 0): the
renderer's trace kernels leave the ray term out when the eye's largest |coordinate| is at most 4 m (PT_BVH_NEAR_EYE, D < 8 m;
every other ray of a path starts on the scene) and rely on exactly this.  Hits at a real incidence of cos < 0.01 (a ray aimed at one triangle of the soup grazes
others) are outside what any finite margin covers (csrc/pt_bvh.hip); they are counted and printed, not asserted: 13 to 19 per
row on the soup, the worst 1.40 x (eps + w) at cos 6.8e-4 at D/m = 1000.
"""
import functools

import numpy as np
import pytest

import lbvh_far as F

RAY_EPS = 1.2e-4          # PT_BVH_RAY_EPS (csrc/pt_kernels.h)
RAYS = 400_000

# (scene, D/m) -> the largest excess / (eps + w) over the hits at cos >= 0.01
MEASURED = {
    ("tile", 1.0): 0.000482, ("tile", 10.0): 0.00069, ("tile", 100.0): 0.00102, ("tile", 1e3): 0.00077, ("tile", 1e4): 0.00166, ("tile", 1e5): 0.00171,
    ("soup", 1.0): 0.0, ("soup", 10.0): 0.0, ("soup", 100.0): 0.0122, ("soup", 1e3): 0.118, ("soup", 1e4): 0.0364, ("soup", 1e5): 0.0595,
}
# (scene, D/m) -> the largest excess / eps over the same hits
SCENE_ONLY = {
    ("tile", 1.0): 0.000994, ("tile", 10.0): 0.0052, ("tile", 100.0): 0.1013, ("soup", 1.0): 0.0, ("soup", 10.0): 0.0, ("soup", 100.0): 1.072,
}


@functools.lru_cache(maxsize=None)
def measure(name, dm):
    """The accepted hits of the edge family at D/m = dm whose REAL incidence (on the triangle that was hit: a ray aimed at one
    triangle of the soup grazes others) has cos >= 0.01, the documented range; what lies below it is counted and reported."""
    import query_oracle as qo

    make, cap = F.SCENES[name]
    tris = make()
    eps = F.BVH_EPS * F.scene_m(tris)
    rays, _ = F.family_edge(tris, cap, dm, np.random.default_rng([ord(c) for c in name] + [int(np.log10(dm)), 77]), RAYS)
    ray, tri, _ = qo.all_hits(tris, rays)
    r6 = qo.get_rays(rays)
    ex = F.excess(tris, r6, ray, tri)
    v = F.verts(tris)[tri]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    cos = np.abs((r6[ray, 3:].astype(np.float64) * nrm).sum(1)) / np.linalg.norm(nrm, axis=1)
    w = RAY_EPS * np.abs(rays[ray, :3].astype(np.float64)).max(1)
    ok = cos >= 0.01
    return {"hits": int(ok.sum()), "rays_hit": len(np.unique(ray[ok])), "over_eps": int((ex[ok] > eps).sum()),
            "scene": float((ex[ok] / eps).max()), "ray": float((ex[ok] / (eps + w[ok])).max()),
            "grazing": int((~ok).sum()), "grazing_ray": float((ex[~ok] / (eps + w[~ok])).max()) if (~ok).any() else 0.0}


def _report(name, dm, m):
    print("%s at D/m = %g: %d accepted hits at cos >= 0.01, largest excess %.4g eps = %.4g of eps + w; %d of them more than eps outside their "
          "box; %d hits at cos < 0.01, the worst %.4g of eps + w" % (name, dm, m["hits"], m["scene"], m["ray"], m["over_eps"], m["grazing"], m["grazing_ray"]))


@pytest.mark.parametrize("dm", F.DISTANCES)
@pytest.mark.parametrize("name", sorted(F.SCENES))
def test_the_margin_with_its_ray_term_covers_every_distance(name, dm):
    m = measure(name, dm)
    _report(name, dm, m)
    assert m["rays_hit"] >= 0.2 * RAYS
    assert MEASURED[(name, dm)] <= 0.5
    assert m["ray"] <= 2 * MEASURED[(name, dm)]


@pytest.mark.parametrize("dm", [1.0, 10.0, 100.0])
@pytest.mark.parametrize("name", sorted(F.SCENES))
def test_the_scene_margin_alone_near_the_scene(name, dm):
    m = measure(name, dm)
    _report(name, dm, m)
    assert m["scene"] <= 2 * SCENE_ONLY[(name, dm)]
    if name == "tile" or dm <= 10.0:      # D/m <= 10 on BOTH scenes: what the renderer relies on when the eye is near the scene
        assert SCENE_ONLY[(name, dm)] <= 0.5


@pytest.mark.parametrize("dm", [1e4, 1e5])
@pytest.mark.parametrize("name", sorted(F.SCENES))
def test_the_scene_margin_alone_is_exposed_far_out(name, dm):
    """Why the margin has a ray term: without it the exact test accepts hits whose box the exact ray does not touch."""
    m = measure(name, dm)
    _report(name, dm, m)
    assert m["over_eps"] > 0 and m["scene"] > 1.0
