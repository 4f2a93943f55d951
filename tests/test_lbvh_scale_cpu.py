"""The oracle's own scale identities, asserted before any device comparison leans on them (no GPU): for the soup scaled by 2^k with
its rays, k = -9 .. 42, the closest hits are the unscaled scene's -- the same triangle, u and v bit for bit, t = t0 x 2^k exactly
-- for every ray at k >= 0, and at k = -9 for every ray none of whose accepted triangles has a det within reach of the literal
threshold 1e-8 once scaled (det scales by 2^2k; those rays are counted, printed and set aside: 563 of the 16 384 rays).
Outside that range the reference's literal det threshold (1e-8) and binary32 overflow thin the hits out; those bands are where a
single rounding decides a hit, and only parity between device and oracle is asserted there (tests/test_gpu_lbvh_scenes.py)."""
import numpy as np
import pytest

import scenes as S


@pytest.fixture(scope="module")
def base():
    import query_oracle as qo

    t, r = S.scaled(0)
    return qo.closest_threads(t, r)


def _stable(k):
    """Rays whose unscaled search cannot meet the reference's literal det threshold when everything is scaled by 2^k: det scales by
    2^2k, so every triangle the exact test accepts for the ray must keep det x 2^2k >= 2 x 1e-8 (det in float64 here; the factor 2
    is far above binary32's rounding of it).  Upwards nothing is gained or lost before binary32 overflows (t ~ scale^3 / scale^2
    in its intermediates: beyond 2^42)."""
    import query_oracle as qo

    t, r = S.scaled(0)
    ray, tri, _ = qo.all_hits(t, r)
    d = qo.get_rays(r)[ray, 3:].astype(np.float64)
    p1, p2, p3 = (t[f][tri, :3].astype(np.float64) for f in ("p1", "p2", "p3"))
    det = ((p2 - p1) * np.cross(d, p3 - p1)).sum(1)
    ok = np.ones(len(r), bool)
    ok[ray[det * 4.0 ** k < 2e-8]] = False
    return ok


@pytest.mark.parametrize("k", S.IDENTITY)
def test_the_oracles_hits_scale_exactly(base, k):
    import query_oracle as qo

    t, r = S.scaled(k)
    w = qo.closest_threads(t, r)
    ok = _stable(k)
    hit = base[:, 1].view(np.int32) >= 0
    print("2^%d: %d of %d rays hit, %d rays set aside (a det within reach of the threshold)" % (k, hit.sum(), len(r), (~ok).sum()))
    assert hit.mean() >= 0.2 and ok[hit].mean() >= 0.9
    if k >= 0:
        assert ok.all()
    assert np.array_equal(w[ok, 1].view(np.int32), base[ok, 1].view(np.int32)), "2^%d: the triangles differ" % k
    assert np.array_equal(w[ok, 2:4].view(np.uint32), base[ok, 2:4].view(np.uint32)), "2^%d: u, v differ" % k
    hit &= ok
    want = base[hit, 0].astype(np.float64) * 2.0 ** k
    assert np.all(want.astype(np.float32).astype(np.float64) == want) and np.array_equal(w[hit, 0], want.astype(np.float32)), "2^%d: t is not t0 x 2^k" % k


def test_the_partial_bands_are_partial(base):
    """the scales outside the identity range keep some hits and lose some, or lose all: the sharpest points of the device test"""
    import query_oracle as qo

    full = int((base[:, 1].view(np.int32) >= 0).sum())
    for k in sorted(set(S.SCALES) - set(S.IDENTITY)):
        t, r = S.scaled(k)
        hits = int((qo.closest_threads(t, r)[:, 1].view(np.int32) >= 0).sum())
        print("2^%d: %d of the unscaled scene's %d hits" % (k, hits, full))
        assert hits < full
