"""The hierarchy checker (tests/bvh_check.py) has teeth: it passes a valid snapshot made by a small numpy reference builder and
rejects every one of a list of single mutations.  No GPU.  The reference builder shares the checker's decoding, eps, grid and
big-triangle rule, so a misreading of the device's format would pass both here: what closes that is the checker's run on the
device's own snapshots (tests/test_gpu_lbvh_scenes.py)."""
import numpy as np
import pytest

import bvh_check as B


def _scene(n=300, seed=8):
    """a soup of small triangles, five that are big by the builder's rule, and one with a non-finite vertex"""
    from oclpathtracer_amd import scene

    rng = np.random.default_rng(seed)
    t = np.zeros(n, scene.TRIANGLE_DTYPE)
    c = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = c + rng.normal(0, 0.05, (n, 3)).astype(np.float32)
    for k in (17, 40, 111, 200, 260):
        t["p2"][k, :3] = t["p1"][k, :3] + np.float32(1.5)
    t["p3"][77, 1] = np.nan
    return t


@pytest.fixture(scope="module")
def snap():
    tris = _scene()
    recs, gmin, gstep, big = B.reference_build(tris)
    return tris, recs, gmin, gstep, big


def test_the_checker_passes_a_valid_hierarchy(snap):
    tris, recs, gmin, gstep, big = snap
    assert list(big) == [17, 40, 111, 200, 260]
    out = B.check(tris, recs, gmin, gstep, big)
    assert out["leaves"] == len(tris) - 5 - 1 and out["nodes"] >= (out["leaves"] + 7) // 8
    # and one over nothing but non-finite triangles, and one over triangles that share a point
    empty = tris[:4].copy()
    empty["p1"][:, 0] = np.inf
    assert B.check(empty, *B.reference_build(empty))["leaves"] == 0
    point = tris[:9].copy()
    for f in ("p1", "p2", "p3"):
        point[f][:, :3] = (1.0, 2.0, 3.0)
    assert B.check(point, *B.reference_build(point))["leaves"] == 9


def _leaf_parents(recs):
    """[(node record, slot, leaf record)] of every leaf child, by a walk from the root"""
    nodes = recs.view(B.NODE).reshape(-1)
    out, todo = [], [0]
    while todo:
        k = todo.pop()
        cm = int(nodes[k]["imask"]) | int(nodes[k]["lmask"])
        for s in range(8):
            if (cm >> s) & 1:
                child = int(nodes[k]["base"]) + bin(cm & ((1 << s) - 1)).count("1")
                if (int(nodes[k]["lmask"]) >> s) & 1:
                    out.append((k, s, child))
                else:
                    todo.append(child)
    return out


def _mutations(snap):
    tris, recs, gmin, gstep, big = snap
    lp = _leaf_parents(recs)
    k, s, child = lp[0]
    last = max((e for e in lp if e[0] == k), key=lambda e: e[1])      # the last leaf slot of the same node

    def mut(f):
        r = recs.copy()
        f(r.view(B.NODE).reshape(-1), r.view(B.LEAF).reshape(-1))
        return tris, r, gmin, gstep, big

    def lower_qhi(n, l): n[k]["qhi"][0][s] -= 1
    def raise_qlo(n, l): n[k]["qlo"][1][s] += 1
    def drop_leaf(n, l):
        n[last[0]]["lmask"] &= ~(1 << last[1]) & 255
        n[last[0]]["qlo"][:, last[1]], n[last[0]]["qhi"][:, last[1]] = 255, 0
    def duplicate_leaf(n, l): l[lp[1][2]] = l[lp[0][2]]
    def swap_index(n, l): l[lp[0][2]]["index"], l[lp[5][2]]["index"] = l[lp[5][2]]["index"], l[lp[0][2]]["index"]
    def base_off(n, l): n[k]["base"] += 1
    def leaf_to_node(n, l):
        n[k]["lmask"] &= ~(1 << s) & 255
        n[k]["imask"] |= 1 << s
    def raise_org(n, l): n[k]["org"][2] += 1

    yield "qhi lowered by 1", mut(lower_qhi)
    yield "qlo raised by 1", mut(raise_qlo)
    yield "a leaf dropped", mut(drop_leaf)
    yield "a leaf duplicated", mut(duplicate_leaf)
    yield "two leaves' indices swapped", mut(swap_index)
    yield "base off by one", mut(base_off)
    yield "a bit moved from lmask to imask", mut(leaf_to_node)
    yield "org raised by 1", mut(raise_org)
    yield "an unsorted big list", (tris, recs, gmin, gstep, np.array([17, 111, 40, 200, 260]))
    yield "a big triangle left in the tree", (tris,) + B.reference_build(tris, keep_in_tree=(111,))
    yield "a big triangle missing from the list", (tris, recs, gmin, gstep, np.array([17, 40, 200, 260]))
    wide = recs.copy()
    nv = wide.view(B.NODE).reshape(-1)
    nv[k]["ex"][0] += 2                                               # a step four times too coarse: every box still contains its triangles
    yield "a node whose step is four times what it needs", (tris, wide, gmin, gstep, big)


def test_every_single_mutation_is_rejected(snap):
    seen = 0
    for name, args in _mutations(snap):
        with pytest.raises(B.BvhError) as e:
            B.check(*args, verbose=False)
        print("%-48s -> %s" % (name, e.value))
        seen += 1
    assert seen == 12


def test_a_cluster_beside_an_outlier():
    """slab541 (scenes.slab(15) and scenes.slab_rays) without a device: the oracle hits with at least 0.5 of the 4 096 rays, at least
    0.1 of the hits on the slab and 0.3 on the boxes; the 540 small triangles are smaller than ONE cell of the 16-bit grid on every axis
    and the margin PT_BVH_EPS x extent is wider than the cluster; and the checker's rules -- tightness included -- can hold on such a
    grid: the reference builder's hierarchy passes them, so a device hierarchy that fails them is the builder's fault, not the rule's"""
    import query_oracle as qo
    import scenes

    tris, rays = scenes.scene("slab541")
    assert len(tris) == 541 and len(rays) == 4096 and "slab541" in scenes.NAMES
    wt = qo.closest_threads(tris, rays)[:, 1].view(np.int32)
    hit = wt >= 0
    slab, boxes = (wt[hit] == 540).mean(), (wt[hit] < 540).mean()
    print("slab541: the oracle hits with %.2f of the rays (camera %.2f, upward %.2f), %.2f of the hits on the slab, %.2f on the boxes"
          % (hit.mean(), hit[:2048].mean(), hit[2048:].mean(), slab, boxes))
    assert hit.mean() >= 0.5 and slab >= 0.1 and boxes >= 0.3
    assert hit[2048:].mean() >= 0.2 and not (wt[2048:] == 540).any(), "the upward rays leave the slab's back and meet the boxes"
    v, finite, lo, hi = B.tri_boxes(tris)
    gmin, gstep = B.reference_grid(v, finite, lo, hi)
    eps = B.scene_eps(v, finite)
    cluster = hi[:540].max(0) - lo[:540].min(0)
    assert np.all(cluster < gstep) and eps > cluster.max() and eps > 2 * gstep.max()
    out = B.check(tris, *B.reference_build(tris))
    assert out["leaves"] == 540 and list(B.big_set(finite, lo, hi)) == [540]
