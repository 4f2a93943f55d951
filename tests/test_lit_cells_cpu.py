"""tests/lit_cells.py reaches what it says it reaches, proved on the CPU from the table alone: every scene takes the form its row
names -- by its triangle count against 256 and PT_BVH_AUTO_MIN, its determinant product against PT_DET_BOUND_MAX and the quad pairing
of the table that is searched --, the eight forms and the fourteen kinds are all there, and the cell's size is the one whose launch
has several waves, workgroups and roulette runs."""
import os
import re

import numpy as np

import lit_cells as lc
import roulette_cases as rc
from conftest import ROOT
from scenes import edge_scene


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


def test_fourteen_kinds_eight_forms():
    assert len(lc.KINDS) == 14 and len({k.name for k in lc.KINDS}) == 14
    assert len({k[1:] for k in lc.KINDS}) == 14
    for k in lc.KINDS:   # list implies rr, rr implies indirect, mis only with indirect
        assert (not k.list or k.rr) and (not k.rr or k.indirect) and (not k.mis or k.indirect), k
    assert sum(not k.indirect for k in lc.KINDS) == 2 and all(sum(k.rr == rr and k.list == lst for k in lc.KINDS if k.indirect) == 4
                                                                for rr, lst in ((False, False), (True, False), (True, True)))
    assert {(f.search, f.bounded, f.quads) for f in lc.FORMS} == {("lbvh", True, 3), ("lbvh", True, 0), ("lbvh", False, 0),
                                                                 ("lds", True, 3), ("lds", True, 0), ("lds", False, 0),
                                                                 ("tiled", True, 0), ("tiled", False, 0)}
    assert len(lc.FORMS) == 8 and 104 <= len(lc.CELLS) == 112 - len(lc.LEFT_OUT)
    for form, kind in lc.LEFT_OUT:
        assert form in {f.name for f in lc.FORMS} and kind in {k.name for k in lc.KINDS}


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
    """the two LBVH scenes at scale 1: 36 big triangles that are quads, and 520 big ones, more than the table holds"""
    one, fifteen = edge_scene("scaled:1,0")[1][0], edge_scene("scaled:15,0")[1][0]
    assert len(lc.big_triangles(one)) == 36 and lc.is_quads(one[lc.big_triangles(one)])
    assert len(lc.big_triangles(fifteen)) == 0 and len(fifteen) == 540


def test_the_cell_is_several_waves_workgroups_and_runs():
    items = lc.W * lc.H * lc.FRAMES
    assert items == 768 and items // 64 == 12 and items // 256 == 3 and items == 3 * rc.rr_run()
    assert (lc.K, lc.B, lc.R, lc.CAP) == (2, 6, 1, 0.25) and (1, 0.25) in rc.BIG_SETTINGS
    s = lc.slots()
    assert len(s) == lc.LISTED == 101 and len(set(s["pixel"].tolist())) == 101 and s["pixel"].max() < lc.W * lc.H
    assert len(set(s["frame"].tolist())) > 3 and (s["frame"] == 0).any() and (np.diff(s["pixel"].astype(np.int64)) < 0).any()
