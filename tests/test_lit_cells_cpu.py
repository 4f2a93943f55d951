"""tests/lit_cells.py reaches what it says it reaches, proved on the CPU from the table alone: every scene takes the form its row
names -- by its triangle count against 256 and PT_BVH_AUTO_MIN, its determinant product against PT_DET_BOUND_MAX and the quad pairing
of the table that is searched --, the eleven forms and the twenty-one kinds are all there (the kinds are ptk_lit_kind_valid's), and the
cell's size is the one whose launch has several waves, workgroups and roulette runs.  Of the three slab forms -- the unbounded forms
that shade -- it proves, on the restatements alone, that the scene sits in its window (above the bound, a finite normal), that first
hits fall on the slab and on the boxes, that paths come back to the slab, that light samples at its vertices are open and occluded, that
no radiance of any kind is non-finite, that resampling changes the samples and that the sky's texels show."""
import itertools
import os
import re

import numpy as np
import pytest

import direct_oracle as do
import env_oracle as eo
import indirect_oracle as io
import lit_cells as lc
import ris_oracle as rs
import roulette_cases as rc
import scenes
from adaptive_support import _expect
from conftest import ROOT
from env_scenes import env_map
from scenes import edge_scene

SLAB_FORMS = [f for f in lc.FORMS if f.name in lc.SHADING_UNBOUNDED]


def _define(name, text):
    return re.search(r"^#define %s\s+(\S+)" % name, text, re.M).group(1)


def test_the_constants_are_the_headers():
    kernels_h = open(os.path.join(ROOT, "oclpathtracer_amd", "csrc", "pt_kernels.h")).read()
    bvh = open(os.path.join(ROOT, "oclpathtracer_amd", "csrc", "pt_bvh.hip")).read()
    assert int(_define("PT_LDS_TRI_MAX", kernels_h)) == lc.LDS_TRI_MAX
    assert int(_define("PT_BVH_AUTO_MIN", kernels_h)) == lc.BVH_AUTO_MIN
    assert int(_define("PT_BVH_BIG_MAX", kernels_h)) == lc.BVH_BIG_MAX
    assert np.float32(_define("PT_DET_BOUND_MAX", kernels_h).rstrip("f")) == lc.DET_BOUND_MAX
    assert np.float32(_define("PT_BVH_BIG_DIV", bvh).rstrip("f")) == lc.BVH_BIG_DIV


def test_twentyone_kinds_eleven_forms():
    assert len(lc.KINDS) == 21 and len({k.name for k in lc.KINDS}) == 21
    assert len({k[1:] for k in lc.KINDS}) == 21
    for k in lc.KINDS:   # list implies rr, rr implies indirect, mis only with indirect
        assert (not k.list or k.rr) and (not k.rr or k.indirect) and (not k.mis or k.indirect), k
    plain = [k for k in lc.KINDS if not k.ris and not k.env]
    assert len(plain) == 14 and plain == list(lc.KINDS[:14])   # (the fourteen kinds of before, as they were)
    assert sum(not k.indirect for k in plain) == 2 and all(sum(k.rr == rr and k.list == lst for k in plain if k.indirect) == 4
                                                           for rr, lst in ((False, False), (True, False), (True, True)))
    ris, env = [k for k in lc.KINDS if k.ris], [k for k in lc.KINDS if k.env]
    assert {k[1:6] for k in ris} == {(False, False, True, False, False), (True, False, True, True, False), (True, True, True, True, False),
                                     (True, False, True, True, True), (True, True, True, True, True)} and len(ris) == 5
    assert {k[1:6] for k in env} == {(False, False, True, False, False), (True, True, True, True, False)} and len(env) == 2
    assert {(f.search, f.bounded, f.quads) for f in lc.FORMS} == {("lbvh", True, 3), ("lbvh", True, 0), ("lbvh", False, 0),
                                                                 ("lds", True, 3), ("lds", True, 0), ("lds", False, 0),
                                                                 ("tiled", True, 0), ("tiled", False, 0)}
    assert [(f.search, f.bounded, f.quads, f.quad) for f in SLAB_FORMS] == [("lds", False, 0, 0), ("tiled", False, 0, 0), ("lbvh", False, 0, 0)]
    assert len(lc.FORMS) == 11 and len(lc.CELLS) == 231 - len(lc.LEFT_OUT) and lc.LEFT_OUT == ()
    for form, kind in lc.LEFT_OUT:
        assert form in {f.name for f in lc.FORMS} and kind in {k.name for k in lc.KINDS}


def test_the_kinds_are_the_ones_the_library_accepts():
    """ptk_lit_kind_valid and ptk_lit_kind_index as csrc/pt_kernels.h states them, restated in lit_cells and compared with the header's
    text; the table's kinds are exactly the accepted ones, so a kind added to the library fails here until it has cells"""
    kernels_h = open(os.path.join(ROOT, "oclpathtracer_amd", "csrc", "pt_kernels.h")).read()
    squeeze = lambda t: re.sub(r"\s+", "", t)
    assert squeeze("struct PtLitKind { bool indirect, mis, power, rr, list, ris, env; };") in squeeze(kernels_h)
    assert squeeze("""return (!k.list || k.rr) && (!k.rr || k.indirect) && (!k.mis || k.indirect) && (!k.ris || (k.power && k.rr == k.indirect)) &&
           (!k.env || (k.power && !k.ris && !k.list && k.rr == k.indirect && k.mis == k.indirect));""") in squeeze(kernels_h)
    assert squeeze("return k.indirect | k.mis << 1 | k.power << 2 | k.rr << 3 | k.list << 4 | k.ris << 5 | k.env << 6;") in squeeze(kernels_h)
    assert int(_define("PT_LIT_KIND_INDICES", kernels_h)) == lc.LIT_KIND_INDICES
    every = [lc.Kind("", *bits) for bits in itertools.product((False, True), repeat=7)]
    valid = {k[1:] for k in every if lc.kind_valid(k)}
    assert len(valid) == 21 and valid == {k[1:] for k in lc.KINDS}
    index = [lc.kind_index(k) for k in lc.KINDS]
    assert len(set(index)) == 21 and max(lc.kind_index(k) for k in every) == lc.LIT_KIND_INDICES - 1 and max(index) < lc.LIT_KIND_INDICES


def test_every_scene_reaches_its_form():
    for f in lc.FORMS:
        tris = edge_scene(f.scene)[1][0]
        assert lc.form_of(tris, f.quad, f.accel) == (f.search, f.bounded, f.quads), f
        n = len(tris)
        if f.search == "lds":
            assert 0 < n <= lc.LDS_TRI_MAX
        elif f.search == "tiled":
            assert lc.LDS_TRI_MAX < n < lc.BVH_AUTO_MIN and f.accel == 1
        else:
            assert n >= lc.BVH_AUTO_MIN or f.accel == 2
        assert (lc.det_bound(tris) <= lc.DET_BOUND_MAX) == f.bounded
        assert len(edge_scene(f.scene)[1][2]) > 0, "the scene has lights"


def test_the_scale_of_the_unbounded_forms_is_the_smallest():
    """times 2^30 the largest |e1|_1 |e2|_1 passes 2e19, times 2^29 it does not"""
    for copies in (1, 10, 15):
        at = {k: lc.det_bound(edge_scene("scaled:%d,%d" % (copies, k))[1][0]) for k in (0, 29, 30)}
        assert abs(float(at[0]) - 62.58) < 0.01 and at[29] <= lc.DET_BOUND_MAX < at[30], at
        assert lc.is_quads(edge_scene("scaled:%d,30" % copies)[1][0])   # (the pairing survives the scale: only the bound is lost)


def test_the_big_tables():
    """the two LBVH scenes at scale 1: 36 big triangles that are quads, and 520 big ones, more than the table holds; beside the slab the
    slab alone is big"""
    one, fifteen = edge_scene("scaled:1,0")[1][0], edge_scene("scaled:15,0")[1][0]
    assert len(lc.big_triangles(one)) == 36 and lc.is_quads(one[lc.big_triangles(one)])
    assert len(lc.big_triangles(fifteen)) == 0 and len(fifteen) == 540
    slab = edge_scene("slab:15")[1][0]
    assert len(slab) == 541 and lc.big_triangles(slab).tolist() == [540]


# ---- the slab forms: unbounded forms that shade ---------------------------------------------------------------------------------------
def _slab_normal_square(tris):
    """|cross(e2, e1)|^2 of the last triangle in binary32, as the triangle test's normalisation forms it"""
    e1 = tris["p2"][-1, :3] - tris["p1"][-1, :3]
    e2 = tris["p3"][-1, :3] - tris["p1"][-1, :3]
    with np.errstate(over="ignore"):
        c = np.cross(e2, e1).astype(np.float32)
        return np.float32((c * c).sum(dtype=np.float32))


@pytest.mark.parametrize("copies", [1, 10, 15])
def test_the_slab_sits_in_its_window(copies):
    """above PT_DET_BOUND_MAX by the slab alone, its normal's square finite in binary32; the twin of L = 2.2e9 sits below the bound"""
    tris, mats, lights, cam = edge_scene("slab:%d" % copies)[1]
    assert len(tris) == 36 * copies + 1 and tris["id"][-1] == len(mats) - 1 and (tris["id"][:-1] < len(mats) - 1).all()
    assert lc.det_bound(tris) > lc.DET_BOUND_MAX >= lc.det_bound(tris[:-1]) and lc.det_bound(tris[-1:]) == lc.det_bound(tris)
    assert np.isfinite(_slab_normal_square(tris)) and _slab_normal_square(tris) > 0
    assert len(lights) == 2 * copies and lights.max() < len(tris) - 1   # (the boxes' emitters as they are; the slab emits nothing)
    twin = edge_scene("slab:%d,bounded" % copies)[1][0]
    assert lc.det_bound(twin) <= lc.DET_BOUND_MAX and lc.form_of(twin, 0, 1)[1] is True
    assert scenes.SLAB_L_BOUNDED < (float(lc.DET_BOUND_MAX) / 4) ** 0.5 < scenes.SLAB_L < (3.4028235e38 / 4) ** 0.25


def _slab_details(scene):
    tris, mats, lights, cam = edge_scene(scene)[1]
    gid, frame = io.all_samples(lc.W, lc.H, lc.FRAMES)
    return io.details(tris, mats, lc.W, lc.H, gid, frame, lc.K, lc.B, lights=lights, cam=cam)


@pytest.mark.parametrize("form", SLAB_FORMS, ids=[f.name for f in SLAB_FORMS])
def test_the_slab_forms_shade(form):
    """what the restatement says of the form's scene at the cell's size: first hits on the slab (>= 0.4) and on the boxes (>= 0.2), paths
    that meet the slab at a later vertex (>= 0.05), light samples at slab vertices open and occluded, no non-finite sample"""
    tris, mats = edge_scene(form.scene)[1][:2]
    mtype, flipped, emissive, reason, end, rad, nonfinite, material = do.once(_slab_details, form.scene)
    slab = len(mats) - 1
    n = len(material)
    first = material[:, 0]
    on_slab, on_boxes, miss = (first == slab).sum() / n, ((first >= 0) & (first != slab)).sum() / n, (first < 0).sum() / n
    later = (material[:, 1:] == slab).any(axis=1).sum() / n
    at_slab = material == slab
    opened, occluded = int((reason[at_slab] == do.R_OPEN).sum()), int((reason[at_slab] == do.R_OCCLUDED).sum())
    print("%s: first hit slab %.2f boxes %.2f miss %.2f; slab later %.2f; light samples at slab vertices open %d occluded %d; non-finite %d"
          % (form.name, on_slab, on_boxes, miss, later, opened, occluded, int(nonfinite.sum())))
    assert on_slab >= 0.4 and on_boxes >= 0.2 and later >= 0.05
    assert opened >= 1 and occluded >= 1
    assert int(nonfinite.sum()) == 0 and np.isfinite(rad).all()


@pytest.mark.parametrize("form", SLAB_FORMS, ids=[f.name for f in SLAB_FORMS])
def test_no_kind_is_non_finite_on_the_slab_forms(form):
    """ZERO non-finite radiance samples in every kind's wanted radiance -- the list kinds' included -- and in the framebuffers"""
    slots = lc.slots()
    for kind in lc.KINDS:
        if kind.list:
            ws, end, start = _expect(form.scene, lc.W, lc.H, slots, lc.FRAMES, lc.K, lc.B, lc.R, lc.CAP, kind.mis, kind.power,
                                     candidates=lc.M if kind.ris else 0)
            assert np.isfinite(ws).all() and np.isfinite(end).all() and np.isfinite(start).all(), (form.name, kind.name)
        else:
            fb, rad = lc.wanted(kind, form.scene)
            assert rad.shape == (lc.FRAMES, lc.W * lc.H, 3) and np.isfinite(rad).all() and np.isfinite(fb).all(), (form.name, kind.name)


@pytest.mark.parametrize("form", SLAB_FORMS, ids=[f.name for f in SLAB_FORMS])
def test_resampling_changes_the_samples_on_the_slab_forms(form):
    """every indirect RIS kind at M = 8 differs from M = 1 in at least 0.2 of its samples (measured: 0.74 - 0.83 beside one box, 0.31 -
    0.36 beside 10 and 15); the direct kind in at least 0.2 of the samples that either render lights -- it has one vertex, and under 10
    and 15 boxes every light sample of most first hits is occluded, 0 for any M (0.15 and 0.08 of ALL its samples differ there, which
    is every lit one)"""
    tris, mats, lights, cam = edge_scene(form.scene)[1]
    gid, frame = io.all_samples(lc.W, lc.H, lc.FRAMES)
    for kind in (k for k in lc.KINDS if k.ris and not k.list):   # (a list kind renders its roulette kind's samples at other frames)
        kw = dict(lights=lights, cam=cam)
        if kind.indirect:
            kw.update(B=lc.B, R=lc.R, cap=lc.CAP, mis=kind.mis)
        one = rs.samples(tris, mats, lc.W, lc.H, gid, frame, lc.K, 1, **kw)
        many = lc.wanted(kind, form.scene)[1].reshape(-1, 3)
        differs = (one.view(np.uint32) != many.view(np.uint32)).any(axis=1)
        share = differs.mean()
        if not kind.indirect:
            # One vertex only: a sample can differ only where a light sample of either render arrives, and under 10 and 15 nested boxes
            # most first hits have every light sample occluded (0 for any M).  The share is taken over the samples either render lights
            lit = ((one != 0) | (many != 0)).any(axis=1) & (do.once(_slab_details, form.scene)[7][:, 0] >= 0)
            print("%s %s: %.2f of all samples differ, %d samples are lit" % (form.name, kind.name, share, lit.sum()))
            assert lit.sum() >= 50, (form.name, kind.name)
            share = differs[lit].mean()
        print("%s %s: M = 8 differs from M = 1 in %.2f of the samples" % (form.name, kind.name, share))
        assert share >= 0.2, (form.name, kind.name)
    slots = lc.slots()
    for kind in (k for k in lc.KINDS if k.ris and k.list):
        ws = {m: _expect(form.scene, lc.W, lc.H, slots, lc.FRAMES, lc.K, lc.B, lc.R, lc.CAP, kind.mis, True, candidates=m)[0] for m in (1, lc.M)}
        share = (ws[1].view(np.uint32) != ws[lc.M].view(np.uint32)).any(axis=2).mean()
        print("%s %s: M = 8 differs from M = 1 in %.2f of the samples" % (form.name, kind.name, share))
        assert share >= 0.2, (form.name, kind.name)


@pytest.mark.parametrize("form", SLAB_FORMS, ids=[f.name for f in SLAB_FORMS])
def test_the_sky_shows_on_the_slab_forms(form):
    """at least 0.05 of each env kind's samples end in a miss whose texel is not the constant sky's 0.45"""
    tris, mats, lights, cam = edge_scene(form.scene)[1]
    gid, frame = io.all_samples(lc.W, lc.H, lc.FRAMES)
    t = env_map(lc.ENV_MAP)
    flat = eo.texels4(t)
    assert not (flat[:, :3] == np.float32(0.45)).all(axis=1).any() and len(np.unique(flat[:, :3], axis=0)) == len(flat)
    for kind in (k for k in lc.KINDS if k.env):
        kw = dict(lights=lights, cam=cam, details=True)
        if kind.indirect:
            kw.update(B=lc.B, R=lc.R, cap=lc.CAP)
        rad, d = eo.samples(tris, mats, t, lc.W, lc.H, gid, frame, lc.K, lc.KE, **kw)
        assert np.array_equal(rad.view(np.uint32), lc.wanted(kind, form.scene)[1].reshape(-1, 3).view(np.uint32))
        mt = d["miss_texel"]
        other = (mt >= 0) & (flat[np.maximum(mt, 0), :3] != np.float32(0.45)).any(axis=-1)
        share = other.any(axis=1).mean()
        print("%s %s: %.2f of the samples end in a miss whose texel is not 0.45" % (form.name, kind.name, share))
        assert share >= 0.05, (form.name, kind.name)


def test_the_cell_is_several_waves_workgroups_and_runs():
    items = lc.W * lc.H * lc.FRAMES
    assert items == 768 and items // 64 == 12 and items // 256 == 3 and items == 3 * rc.rr_run()
    assert (lc.K, lc.B, lc.R, lc.CAP) == (2, 6, 1, 0.25) and (1, 0.25) in rc.BIG_SETTINGS
    s = lc.slots()
    assert len(s) == lc.LISTED == 101 and len(set(s["pixel"].tolist())) == 101 and s["pixel"].max() < lc.W * lc.H
    assert len(set(s["frame"].tolist())) > 3 and (s["frame"] == 0).any() and (np.diff(s["pixel"].astype(np.int64)) < 0).any()
