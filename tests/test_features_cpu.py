"""The first-hit feature oracle (tests/feature_oracle.c) against the restatements that exist, the merge of two calls' moments, the proofs
that the inputs of tests/test_gpu_features.py reach their edges -- each a condition on the oracle alone -- and the parameter block's
layout.  No GPU."""
import ctypes

import numpy as np

import feature_cases as fc
import feature_oracle as fo
import moments_oracle as mom
import query_oracle
from conftest import assert_fb_equal


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_oracle_is_the_camera_and_query_restatements(cornell):
    """Cornell 40 x 24, frames 0 and 7: t, the normal and the material of every sample equal the closest hit (query_oracle.closest) of
    the camera restatement's rays (query_oracle.camera_rays) bit for bit -- the normal up to the sign :243 gives it, the material
    through the clamp -- and a miss is zeros in all four arrays."""
    tris, mats = cornell
    for frame in (0, 7):
        s = fo.samples(tris, mats, fc.W, fc.H, 1, frame_begin=frame)
        hits = query_oracle.closest(tris, query_oracle.camera_rays(fc.W, fc.H, frame))
        tri = hits[:, 1].view(np.int32)
        hit = tri >= 0
        assert 0 < int(hit.sum()) < len(hit)
        assert np.array_equal(s.tri[0], tri)
        assert np.array_equal(_bits(s.depth[0][hit, 0]), _bits(hits[hit, 0])), "t"
        assert np.array_equal(_bits(s.normal[0][hit]) & 0x7fffffff, _bits(hits[hit, 8:11]) & 0x7fffffff), "|normal|"
        mid = hits[hit, 7].view(np.int32)
        assert np.array_equal(s.id[0][hit], mid)
        assert np.array_equal(_bits(s.albedo[0][hit]), _bits(mats["albedo"][mid, :3])), "albedo"
        assert np.array_equal(_bits(s.emission[0][hit]), _bits(np.float32(1.0) * mats["emissive"][mid, :3] * np.float32(3.0))), "emission"
        assert np.all(s.depth[0][hit, 1] == 1.0) and np.all(s.depth[0][hit, 2] > 0.0)
        for a in (s.albedo, s.normal, s.depth, s.emission):
            assert not _bits(a[0][~hit]).any(), "a miss is +0 everywhere"
        # the sign: n faces the ray
        d = query_oracle.get_rays(query_oracle.camera_rays(fc.W, fc.H, frame))[:, 3:]
        assert np.all((s.normal[0][hit].astype(np.float64) * d[hit]).sum(axis=1) < 0.0)


def test_two_calls_merge_into_one(cornell):
    """the moments of a frames, then b frames from frame a on, equal those of one call of a + b frames, per feature"""
    a, b = 3, 4
    whole = fc.oracle("cornell", frames=a + b)
    tris, mats, _ = fc.case("cornell")
    first = fo.samples(tris, mats, fc.W, fc.H, a)
    second = fo.samples(tris, mats, fc.W, fc.H, b, frame_begin=a)
    for name in fo.FEATURES:
        want = mom.accumulate(getattr(whole, name))
        got = mom.accumulate(getattr(second, name), mom.accumulate(getattr(first, name)))
        assert got.tobytes() == want.tobytes(), name
        assert np.array_equal(_bits(np.concatenate([getattr(first, name), getattr(second, name)])), _bits(getattr(whole, name))), name


# ---- the inputs reach their edges: conditions on the oracle alone ------------------------------------------------------------------
def test_from_behind_negates_every_normal():
    """The triangle test is one-sided (:100 passes det = dot(d, cross(e2, e1)) > 0 only), so the HitRecord normal of every hit points
    along the ray and :243 negates it on EVERY hit, from any camera: tests/test_direct_cpu.py proves it for direct illumination, and it
    holds here.  An un-negated hit is reached by no ray of any input of this suite -- from behind the box as little as from the front
    (measured: 1110 hits, 1110 negated, at 40 x 24 x 2).  What the case checks is the sign the device gives the stored normal."""
    s = fc.oracle("from_behind")
    hit = s.tri >= 0
    print("from_behind: hits %d, negated %d, misses %d" % (int(hit.sum()), int(s.flipped.sum()), int((~hit).sum())))
    assert int(s.flipped.sum()) >= 500
    assert np.array_equal(s.flipped == 1, hit)
    for name in ("cornell", "soup", "non_finite"):
        o = fc.oracle(name)
        assert np.array_equal(o.flipped == 1, o.tri >= 0), name


def test_odd_materials_has_ids_outside_the_table():
    """hits whose id lies below 0 and hits whose id lies above the table, and what the clamp makes of them"""
    tris, mats, _ = fc.case("odd_materials")
    s = fc.oracle("odd_materials")
    below, above = s.id == fc.BELOW, s.id == fc.ABOVE
    hit = s.tri >= 0
    print("odd_materials: hits %d, id below %d, id above %d" % (int(hit.sum()), int((below & hit).sum()), int((above & hit).sum())))
    assert int((below & hit).sum()) >= 50 and int((above & hit).sum()) >= 50
    assert np.array_equal(_bits(s.albedo[below & hit]), np.broadcast_to(_bits(mats["albedo"][0, :3]), s.albedo[below & hit].shape))
    assert np.array_equal(_bits(s.albedo[above & hit]), np.broadcast_to(_bits(mats["albedo"][-1, :3]), s.albedo[above & hit].shape))
    assert np.isnan(s.albedo).any(), "the NaN albedo of material 12 is stored as it is"
    assert (s.albedo < 0).any(), "... and the negative one of material 1"


def test_other_type_keeps_its_albedo():
    """materials of type 3 are met, and their albedo is stored whatever the type"""
    tris, mats, _ = fc.case("other_type")
    s = fc.oracle("other_type")
    hit = s.tri >= 0
    types = mats["type"][s.id[hit]]
    assert int((types == 3).sum()) >= 500
    assert np.array_equal(_bits(s.albedo[hit]), _bits(mats["albedo"][s.id[hit], :3]))


def test_non_finite_has_nan_records():
    """No triangle of scenes.non_finite is ever hit (t is NaN and `t > 0` fails), so it is the overflowing triangle that gives the NaN
    records: the normal's y and with it -dot(n, d); t, the coverage weight, albedo and emission stay finite.  The moments reject such a
    sample whole."""
    tris, mats, _ = fc.case("non_finite")
    s = fc.oracle("non_finite")
    bad = np.isnan(s.normal).any(axis=2)
    print("non_finite: hits %d, NaN records %d" % (int((s.tri >= 0).sum()), int(bad.sum())))
    assert int(bad.sum()) >= 100
    assert np.array_equal(bad, s.tri == len(tris) - 1)
    assert not (s.tri[s.tri >= 0] >= 36).any() or set(np.unique(s.tri[s.tri >= 36])) == {len(tris) - 1}
    assert np.array_equal(np.isnan(s.normal[bad]), np.broadcast_to([False, True, False], s.normal[bad].shape))
    assert np.array_equal(np.isnan(s.depth[bad]), np.broadcast_to([False, False, True], s.depth[bad].shape))
    assert np.isfinite(s.albedo).all() and np.isfinite(s.emission).all()
    assert int((~bad & (s.tri >= 0)).sum()) >= 100, "finite hits beside them"
    m = mom.accumulate(s.normal)
    assert int(m["rejected"].sum()) == int(bad.sum())


def test_small_images_have_hits_and_misses():
    """5 x 13 x 5 is 325 samples, five waves and five lanes; 1 x 1 x 4 a single lane.  From the reference camera a 5 x 13 image sees
    nothing but the box (every sample hits); from behind the box the same image has both hits and misses."""
    s = fc.oracle("cornell", 5, 13, 5)
    assert int((s.tri >= 0).sum()) == 5 * 13 * 5
    b = fc.oracle("from_behind", 5, 13, 5)
    hit = b.tri >= 0
    print("5 x 13 x 5 from behind: hits %d, misses %d" % (int(hit.sum()), int((~hit).sum())))
    assert int(hit.sum()) >= 20 and int((~hit).sum()) >= 20
    one = fc.oracle("cornell", 1, 1, 4)
    assert one.depth.shape == (4, 1, 3) and int((one.tri >= 0).sum()) == 4


def test_the_soups_and_the_lens_are_seen():
    """Hits on the LBVH scenes, and a lens that moves the samples.  with_big is a sparse scene of slivers (measured: 22 hits of 1920
    samples, 12 of them on big triangles): its misses are compared bit for bit as well, so a wrongly found triangle shows on any sample."""
    for name, floor in (("soup", 400), ("with_big", 15)):
        s = fc.oracle(name)
        hit = s.tri >= 0
        print("%s: hits %d of %d, triangles met %d" % (name, int(hit.sum()), hit.size, len(np.unique(s.tri[hit]))))
        assert floor <= int(hit.sum()) < hit.size
    tris = fc.case("with_big")[0]
    big = np.flatnonzero(np.abs(tris["p2"][:, 0] - tris["p1"][:, 0]) >= 1.4)
    on_big = np.isin(fc.oracle("with_big").tri, big)
    assert len(big) == 64 and 5 <= int(on_big.sum()) < int((fc.oracle("with_big").tri >= 0).sum()), "big and small triangles are met"
    lens, pin = fc.oracle("lens", frames=3), fc.oracle("cornell", frames=3)
    assert int((_bits(lens.depth) != _bits(pin.depth)).any(axis=2).sum()) > 1000
    assert np.array_equal(lens.tri >= 0, lens.depth[..., 1] == 1.0)


def test_the_slab_scenes_show_the_slab():
    """the unbounded scenes of tests/test_gpu_features.py take their search unbounded; the slab's own material (the table's last, met on
    no box) shows in at least 0.4 of the samples -- its id and albedo stored, its depth a hit's -- the boxes in 0.2, and no normal is NaN"""
    import lit_cells as lc

    for search, name, accel in fc.SLAB_FORMS:
        tris, mats, cam = fc.case(name)
        assert lc.form_of(tris, 0, accel)[:2] == (search, False)
        s = fc.oracle(name, fc.SLAB_W, fc.SLAB_H)
        slab = s.tri == len(tris) - 1
        boxes = (s.tri >= 0) & ~slab
        print("%s: slab %.2f, boxes %.2f, misses %.2f of the samples" % (name, slab.mean(), boxes.mean(), (s.tri < 0).mean()))
        assert slab.mean() >= 0.4 and boxes.mean() >= 0.2 and (s.tri < 0).any()
        assert np.all(s.id[slab] == len(mats) - 1) and not np.any(s.id[boxes] == len(mats) - 1)
        assert np.array_equal(_bits(s.albedo[slab]), np.broadcast_to(_bits(mats["albedo"][-1, :3]), s.albedo[slab].shape))
        assert np.all(s.depth[slab][:, 1] == 1.0) and np.all(s.depth[slab][:, 0] > 0.0) and np.isfinite(s.depth).all()
        assert not np.isnan(s.normal).any() and np.all(s.normal[slab] == np.float32([0.0, 1.0, 0.0]))


def test_stripes_are_the_whole_image_rows():
    """stripe_rows = 5, n_ranks = 3, rank = 1 of 24 rows: rows 5-9 and 20-23, nine rows, with the whole image's samples"""
    part = fc.oracle("cornell", stripe_rows=5, n_ranks=3, rank=1)
    whole = fc.oracle("cornell")
    rows = [r for r in range(fc.H) if (r // 5) % 3 == 1]
    assert rows == [5, 6, 7, 8, 9, 20, 21, 22, 23]
    gids = (np.array(rows)[:, None] * fc.W + np.arange(fc.W)[None, :]).reshape(-1)
    for name in fo.FEATURES:
        assert_fb_equal(getattr(part, name), getattr(whole, name)[:, gids], name)


def test_the_block_is_64_bytes_and_the_header_is_bound():
    from oclpathtracer_amd import shim
    from test_shim_abi import test_header_symbols_are_exported_and_bound

    assert ctypes.sizeof(shim.FeatureParams) == 64
    assert shim.FeatureParams.reserved.offset == 36 and shim.FeatureParams.reserved.size == 28
    assert "pt_render_features" in shim.SIGNATURES
    assert (shim.PT_FEATURE_ALBEDO, shim.PT_FEATURE_NORMAL, shim.PT_FEATURE_DEPTH, shim.PT_FEATURE_EMISSION) == (1, 2, 4, 8)
    test_header_symbols_are_exported_and_bound()
