"""An independent check of the hierarchy the GPU built (pt_bvh_snapshot): numpy only.  TEST INFRASTRUCTURE.

The builder (csrc/pt_bvh.hip, pt_bvh8_write) verifies its boxes by decoding them with the expression the traversal uses; nothing
else looked at the result but pixels and rays.  check() takes the caller's triangle records and the snapshot and verifies

  structure    walking from record 0, every record index is below the records in use and is reached exactly once; a node's node
               and leaf masks are disjoint; the child in slot s is record base + popcount((imask | lmask) & ((1 << s) - 1))
               (csrc/pt_kernels.h); empty slots hold the inverted box (255, 0); step exponents lie in 1..254; the leaves'
               `index` values, the list of big triangles and the triangles with a non-finite vertex partition 0 .. n-1; the big
               list is ascending, has at most 64 entries and is exactly the set pt_bvh.hip defines -- finite triangles whose
               longest box side exceeds the scene's longest side / 16, or nothing when that set has more than 64 members; a
               leaf holds p1, e1 = p2 - p1, e2 = p3 - p1 of its triangle in binary32, bit for bit (pt_prep_kernel:
               GenerateColors.cl:92-93, one subtraction per component);
  containment  every child box, decoded exactly as the traversal does -- fma(q, 2^(ex-127), fma(org, gstep, gmin)), one rounding
               per fma -- contains the box, grown by eps = PT_BVH_EPS x (largest |coordinate|) + 1e-30 in binary32, of EVERY
               triangle below that child;
  tightness    (what pt_bvh8_write's construction guarantees, so that a builder cannot pass with scene-sized boxes): a decoded
               bound lies within one step (x (1 + 2^-8): SLACK) plus one ulp of the bound it covers; a node's origin lies within one grid
               step plus one ulp below its children's lower corner; step <= 4 x (extent / 255), extent = the children's top - the origin.

The fmas are evaluated in float64 and rounded once to binary32; that is exact when the product and the addend fit 53 bits
together, which is asserted (an exponent precondition) wherever it is used.
"""
from __future__ import annotations

import numpy as np

BVH_EPS = np.float32(1.2e-4)      # PT_BVH_EPS
BIG_DIV = np.float32(16.0)        # PT_BVH_BIG_DIV
BIG_MAX = 64                      # PT_BVH_BIG_MAX
# The builder finds a position as floor((bound - origin) / step) in binary32 before it corrects by decoding, downwards (lower bounds) or
# upwards (upper bounds) only: the difference's rounding, at most 2^-24 of 65 536 grid steps (2^-16 of 256 box steps), can cost one
# position when the quotient lies that close above an integer.  "Within one step" is therefore one step x (1 + 2^-8), plus one ulp.
SLACK = 1.0 + 2.0 ** -8

NODE = np.dtype([("org", "<u2", 3), ("ex", "u1", 3), ("imask", "u1"), ("lmask", "u1"), ("pad", "u1"), ("base", "<u4"),
                 ("qlo", "u1", (3, 8)), ("qhi", "u1", (3, 8))])
LEAF = np.dtype([("p1", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("index", "<u4"), ("pad", "<f4", 6)])
assert NODE.itemsize == 64 and LEAF.itemsize == 64


class BvhError(AssertionError):
    pass


def _need(cond, msg, *args):
    if not cond:
        raise BvhError(msg % args)


def tri_boxes(tris):
    """float32 vertices [n, 3, 3], finite [n], box lo / hi [n, 3] of the caller's records"""
    v = np.stack([tris["p1"][:, :3], tris["p2"][:, :3], tris["p3"][:, :3]], 1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return v, np.isfinite(v).all((1, 2)), v.min(1), v.max(1)


def scene_eps(v, finite) -> np.float32:
    m = np.float32(np.abs(v[finite]).max()) if finite.any() else np.float32(0.0)
    return np.float32(np.float32(BVH_EPS * m) + np.float32(1e-30))


def big_set(finite, lo, hi):
    """the triangles pt_bvh.hip keeps out of the hierarchy, ascending"""
    if not finite.any():
        return np.zeros(0, np.int64)
    ext = np.float32((hi[finite].max(0) - lo[finite].min(0)).max())
    if not ext > 0:
        return np.zeros(0, np.int64)
    thr = np.float32(ext / BIG_DIV)
    with np.errstate(invalid="ignore"):
        cand = finite & ((hi - lo).max(1) > thr)
    return np.flatnonzero(cand) if cand.sum() <= BIG_MAX else np.zeros(0, np.int64)


def fma32(q, step_exp, addend, qbits, what):
    """float32(q x 2^step_exp + addend) with ONE rounding: q an integer array below 2^qbits, addend float32.  Asserts that the
    float64 sum is exact."""
    q = np.asarray(q, np.float64)
    e = np.asarray(step_exp, np.int64)
    a = np.asarray(addend, np.float32)
    _, ea = np.frexp(a.astype(np.float64))
    ea = ea.astype(np.int64)
    top = np.where(a != 0, np.maximum(ea, e + qbits), e + qbits) + 1
    bot = np.where(a != 0, np.minimum(ea - 24, e), e)
    _need(np.all((top - bot <= 52) | (q == 0)), "%s: the exponent precondition of the exact decoding does not hold", what)
    return (q * np.ldexp(1.0, e) + a.astype(np.float64)).astype(np.float32)


def _popcount8(x):
    return np.unpackbits(np.asarray(x, np.uint8)[..., None], axis=-1).sum(-1).astype(np.int64)


def check(tris, records, grid_min, grid_step, big, verbose=True):
    """Raises BvhError on the first violation; returns {"nodes", "leaves", "raised_share", "depth"}."""
    rec = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(records).tobytes(), np.uint8))
    _need(rec.size % 64 == 0 and rec.size >= 64, "the snapshot holds no whole record")
    R = rec.size // 64
    nodes, leaves = rec.view(NODE), rec.view(LEAF)
    n = len(tris)
    v, finite, tlo, thi = tri_boxes(tris)
    eps = scene_eps(v, finite)
    gmin, gstep = np.asarray(grid_min, np.float32), np.asarray(grid_step, np.float32)
    gm, ge = np.frexp(gstep.astype(np.float64))
    _need(np.all(gm == 0.5) and np.all(gstep > 0), "grid steps %r are not powers of two", gstep.tolist())
    ge = ge.astype(np.int64) - 1

    # ---- the big list ----
    big = np.asarray(big, np.int64).reshape(-1)
    _need(len(big) <= BIG_MAX, "%d big triangles, more than %d", len(big), BIG_MAX)
    _need(np.all(np.diff(big) > 0), "the big list is not ascending: %r", big.tolist())
    want_big = big_set(finite, tlo, thi)
    _need(np.array_equal(big, want_big), "the big list %r is not the set the builder defines, %r", big.tolist(), want_big.tolist())

    # ---- structure: a level-by-level walk from record 0 ----
    kind = np.zeros(R, np.int8)          # 1 node, 2 leaf
    kind[0] = 1
    frontier = np.array([0], np.int64)
    pairs = []                           # per level: (parent, child, slot)
    depth = 0
    while len(frontier):
        depth += 1
        _need(depth <= 70, "the walk is deeper than any hierarchy over 64-bit keys")
        nd = nodes[frontier]
        im, lm = nd["imask"].astype(np.int64), nd["lmask"].astype(np.int64)
        _need(np.all((im & lm) == 0), "node %d: imask & lmask != 0", int(frontier[np.flatnonzero(im & lm)[0]]) if np.any(im & lm) else -1)
        _need(np.all((nd["ex"] >= 1) & (nd["ex"] <= 254)), "a step exponent outside 1..254")
        cm = im | lm
        P, C, S, K = [], [], [], []
        for s in range(8):
            has = ((cm >> s) & 1) == 1
            empty = ~has
            _need(np.all(nd["qlo"][empty][:, :, s] == 255) and np.all(nd["qhi"][empty][:, :, s] == 0),
                  "an empty slot %d does not hold the inverted box (255, 0)", s)
            child = nd["base"].astype(np.int64)[has] + _popcount8(cm[has] & ((1 << s) - 1))
            P.append(frontier[has]); C.append(child); S.append(np.full(has.sum(), s, np.int64))
            K.append(np.where(((im[has] >> s) & 1) == 1, 1, 2))
        P, C, S, K = (np.concatenate(x) for x in (P, C, S, K))
        _need(np.all(C < R), "a child index %d is not below the %d records in use", int(C.max()) if len(C) else 0, R)
        _need(len(np.unique(C)) == len(C) and np.all(kind[C] == 0), "a record is reached more than once")
        kind[C] = K
        pairs.append((P, C, S))
        frontier = C[K == 1]
    _need(np.all(kind != 0), "%d records in use are never reached (first: %d)", int((kind == 0).sum()), int(np.argmin(kind != 0)))

    # ---- the leaves: a partition of the triangles, and the prepared records ----
    is_leaf = kind == 2
    idx = leaves["index"][is_leaf].astype(np.int64)
    _need(np.all(idx < n), "a leaf's index %d is not below %d triangles", int(idx.max()) if len(idx) else 0, n)
    everyone = np.sort(np.concatenate([idx, big, np.flatnonzero(~finite)]))
    _need(np.array_equal(everyone, np.arange(n)), "leaves, big list and non-finite triangles do not partition 0..%d: %d entries, %d distinct",
          n - 1, len(everyone), len(np.unique(everyone)))
    lf = leaves[is_leaf]
    for name, want in (("p1", v[idx, 0]), ("e1", v[idx, 1] - v[idx, 0]), ("e2", v[idx, 2] - v[idx, 0])):
        same = (np.ascontiguousarray(lf[name]).view(np.uint32) == np.ascontiguousarray(want, np.float32).view(np.uint32)).all(1)
        _need(np.all(same), "leaf of triangle %d: %s is not the caller's record's", int(idx[np.argmin(same)]) if len(idx) else -1, name)

    # ---- the boxes below every record, bottom-up ----
    sub_lo = np.full((R, 3), np.inf, np.float32)
    sub_hi = np.full((R, 3), -np.inf, np.float32)
    where_leaf = np.flatnonzero(is_leaf)
    sub_lo[where_leaf] = tlo[idx] - eps
    sub_hi[where_leaf] = thi[idx] + eps
    for P, C, S in reversed(pairs):
        np.minimum.at(sub_lo, P, sub_lo[C])
        np.maximum.at(sub_hi, P, sub_hi[C])
    childless = (kind == 1) & ~np.isfinite(sub_lo[:, 0])
    _need(childless.sum() == 0 or (R == 1 and childless[0]), "a node other than the root of an empty hierarchy has no children")
    sub_lo[childless], sub_hi[childless] = gmin, gmin

    # ---- containment and tightness ----
    raised = np.zeros(R, bool)
    is_node = np.flatnonzero(kind == 1)
    nd = nodes[is_node]
    org = np.stack([fma32(nd["org"][:, a], ge[a], np.broadcast_to(gmin[a], len(nd)), 16, "a node origin") for a in range(3)], 1)
    org64, lo64, hi64 = org.astype(np.float64), sub_lo[is_node].astype(np.float64), sub_hi[is_node].astype(np.float64)
    step = np.ldexp(1.0, nd["ex"].astype(np.int64) - 127)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    bad = org64 > lo64
    _need(not bad.any(), "node %d: its origin lies above its children's lower corner", int(is_node[np.argmax(bad.any(1))]))
    bad = org64 < lo64 - gstep.astype(np.float64) * SLACK - ulp(lo64)
    _need(not bad.any(), "node %d: its origin lies more than a grid step below its children's lower corner", int(is_node[np.argmax(bad.any(1))]))
    ext = hi64 - org64
    has_kids = ~childless[is_node]
    bad = (step > np.maximum(4.0 * ext / 255.0 * (1 + 1e-6), 2.0 ** -126)) & has_kids[:, None]
    _need(not bad.any(), "node %d: a step above 4 x extent / 255", int(is_node[np.argmax(bad.any(1))]))
    raised[is_node] = ((step > 2.0 * ext / 255.0 * (1 + 1e-6)) & (step > 2.0 ** -126)).any(1) & has_kids
    slot_of = np.full(R, -1, np.int64)
    slot_of[is_node] = np.arange(len(is_node))
    for P, C, S in pairs:
        if not len(P):
            continue
        k = slot_of[P]
        pn = nodes[P]
        for a in range(3):
            e = pn["ex"][:, a].astype(np.int64) - 127
            dlo = fma32(pn["qlo"][np.arange(len(P)), a, S], e, org[k, a], 8, "a child's lower bound").astype(np.float64)
            dhi = fma32(pn["qhi"][np.arange(len(P)), a, S], e, org[k, a], 8, "a child's upper bound").astype(np.float64)
            clo, chi = sub_lo[C, a].astype(np.float64), sub_hi[C, a].astype(np.float64)
            st = np.ldexp(1.0, e)
            for cond, text in ((dlo > clo, "lower bound lies inside the triangles' boxes below it"),
                               (dhi < chi, "upper bound lies inside the triangles' boxes below it"),
                               (dlo < clo - st * SLACK - ulp(clo), "lower bound lies more than a step below what it covers"),
                               (dhi > chi + st * SLACK + ulp(chi), "upper bound lies more than a step above what it covers")):
                if cond.any():
                    j = int(np.argmax(cond))
                    raise BvhError("node %d, slot %d (record %d), axis %d: the decoded %s (decoded [%r, %r], needed [%r, %r], step %r)"
                                   % (int(P[j]), int(S[j]), int(C[j]), a, text, dlo[j], dhi[j], clo[j], chi[j], st[j]))
    out = {"nodes": int((kind == 1).sum()), "leaves": int(is_leaf.sum()), "depth": depth,
           "raised_share": float(raised[is_node].mean()) if len(is_node) else 0.0}
    if verbose:
        print("hierarchy ok: %d triangles, %d nodes, %d leaves, %d big, %d levels; the retry loop raised the step of %.2f %% of the nodes"
              % (n, out["nodes"], out["leaves"], len(big), depth, 100 * out["raised_share"]))
    return out


# ---- a small reference builder for the checker's own test (no GPU): sort by centre, groups of eight, outward quantisation --------
def reference_grid(v, finite, lo, hi):
    """PtBvhGrid as pt_bvh_grid_kernel makes it"""
    eps = scene_eps(v, finite)
    gmin, gstep = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a in range(3):
        l, h = (np.float32(lo[finite, a].min()), np.float32(hi[finite, a].max())) if finite.any() else (np.float32(0), np.float32(0))
        gmin[a] = np.float32(l - np.float32(2) * eps)
        ext = np.float32(np.float32(h - l) + np.float32(4) * eps)
        e2 = int(np.frexp(np.float32(ext / np.float32(65535.0)))[1]) if ext > 0 else -126
        gstep[a] = np.ldexp(np.float32(1), min(max(e2 + 127, 1), 254) - 127)
    return gmin, gstep


def reference_build(tris, keep_in_tree=()):
    """(records uint8 [R, 64], grid_min, grid_step, big) of a valid hierarchy over `tris`.  keep_in_tree: big triangles that
    stay in the tree and off the big list (an INVALID snapshot the checker must reject)."""
    v, finite, lo, hi = tri_boxes(tris)
    eps = scene_eps(v, finite)
    gmin, gstep = reference_grid(v, finite, lo, hi)
    ge = (np.frexp(gstep.astype(np.float64))[1] - 1).astype(np.int64)
    big = np.array([b for b in big_set(finite, lo, hi) if b not in set(keep_in_tree)], np.int64)
    inside = np.flatnonzero(finite & ~np.isin(np.arange(len(tris)), big))
    cen = (lo[inside] + hi[inside]).astype(np.float64)
    order = inside[np.lexsort((cen[:, 2], cen[:, 1], cen[:, 0]))]
    # the tree: ("leaf", tri) or ("node", [children]); boxes of float32
    level = [("leaf", int(t), lo[t] - eps, hi[t] + eps) for t in order]
    mk = lambda g: ("node", g, np.min([c[2] for c in g], 0), np.max([c[3] for c in g], 0))
    while level and not (len(level) == 1 and level[0][0] == "node"):
        level = [mk(level[k: k + 8]) for k in range(0, len(level), 8)]
    root = level[0] if level else ("node", [], gmin.copy(), gmin.copy())
    queue, nxt = [(root, 0)], 1
    out = {}
    while queue:
        (_, kids, nlo, nhi), me = queue.pop(0)
        base = nxt
        nxt += len(kids)
        o = np.zeros(1, NODE)[0]
        o["base"] = base
        o["qlo"][:], o["qhi"][:] = 255, 0
        for s, c in enumerate(kids):
            if c[0] == "leaf":
                o["lmask"] |= 1 << s
                r = np.zeros(1, LEAF)[0]
                t = c[1]
                r["p1"], r["e1"], r["e2"], r["index"] = v[t, 0], v[t, 1] - v[t, 0], v[t, 2] - v[t, 0], t
                out[base + s] = r.tobytes()
            else:
                o["imask"] |= 1 << s
                queue.append((c, base + s))
        for a in range(3):
            dec = lambda q, e, add, bits: float(fma32(np.array([q]), np.array([e]), np.array([add], np.float32), bits, "reference")[0])
            q16 = int(min(max(np.floor((float(nlo[a]) - float(gmin[a])) / float(gstep[a])), 0), 65535))
            while q16 > 0 and dec(q16, ge[a], gmin[a], 16) > nlo[a]:
                q16 -= 1
            org = np.float32(dec(q16, ge[a], gmin[a], 16))
            o["org"][a] = q16
            ext = np.float32(nhi[a] - org)
            be = min(max((int(np.frexp(np.float32(ext / np.float32(255.0)))[1]) if ext > 0 else -126) + 127, 1), 254)
            while True:
                ok = True
                for s, c in enumerate(kids):
                    ql = int(min(max(np.floor((float(c[2][a]) - float(org)) / 2.0 ** (be - 127)), 0), 255))
                    qh = int(min(max(np.ceil((float(c[3][a]) - float(org)) / 2.0 ** (be - 127)), 0), 255))
                    while ql > 0 and dec(ql, be - 127, org, 8) > c[2][a]:
                        ql -= 1
                    while qh < 255 and dec(qh, be - 127, org, 8) < c[3][a]:
                        qh += 1
                    ok = ok and dec(ql, be - 127, org, 8) <= c[2][a] and dec(qh, be - 127, org, 8) >= c[3][a]
                    o["qlo"][a][s], o["qhi"][a][s] = ql, qh
                if ok or be >= 254:
                    break
                be += 1
            o["ex"][a] = be
        out[me] = o.tobytes()
    recs = np.frombuffer(b"".join(out[k] for k in range(nxt)), np.uint8).reshape(-1, 64).copy()
    return recs, gmin, gstep, big
