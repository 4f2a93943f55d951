"""Every lit kernel once on the MI355X, bit for bit: the 21 kinds of lit render under the 11 forms of the search (tests/lit_cells.py),
one kernel instantiation per cell.  Each cell's framebuffer and sample workspace (the radiance before the fold) are compared with the
restatements the lit tests use (direct_oracle, indirect_oracle, mis_oracle, power_oracle, roulette_oracle, ris_oracle, env_oracle), NaN
positions equal.  A launcher that picked another cell's kernel -- the plain estimator for MIS with the power choice on a tiled table,
say -- shows here; on the three slab forms an unbounded kernel that shades, samples a light or folds wrongly shows as well.

tests/test_lit_cells_cpu.py proves that each scene takes its form.  On the device the LBVH forms are asserted through
pt_bvh_snapshot: a hierarchy stands for the scene, and the triangles kept out of it -- the table the two-pass search runs over -- are
the ones the table predicts, quads or none.  Whether the table search is the LDS or the tiled one, packed or not, bounded or not, the
library does not report: it follows from the triangle count, the pairing and the determinant product alone (pt_shim.hip:
prepare_search, ensure_prep; pt_kernels.hip: the launchers), which the CPU test evaluates."""
import ctypes

import numpy as np
import pytest

import lit_cells as lc
from adaptive_support import PixelBuffers, _run_list
from conftest import assert_fb_equal
from env_scenes import env_map
from gpu_support import lit_with_samples, options
from oclpathtracer_amd import shim
from oclpathtracer_amd.environment import Environment
from oclpathtracer_amd.indirect import Roulette
from scenes import edge_scene

pytestmark = pytest.mark.gpu


def _render(device, kind, scene4, sky):
    kw = dict(light_choice="power" if kind.power else "uniform")
    if kind.ris:
        kw.update(candidates=lc.M)
    if kind.env:
        kw.update(environment=sky, env_samples=lc.KE)
    if kind.indirect:
        kw.update(max_bounces=lc.B, mis=kind.mis)
    if kind.rr:
        kw.update(roulette=Roulette(lc.R, lc.CAP))
    return lit_with_samples(device, scene4, lc.W, lc.H, lc.FRAMES, lc.K, **kw)


def _assert_lbvh(device, form, tris):
    """the hierarchy of this scene stands, and what it keeps out is the table the form names"""
    info = shim.BvhInfo()
    big = np.zeros(shim.PT_BVH_SNAPSHOT_BIG_MAX, np.int32)
    shim.check(shim.load().pt_bvh_snapshot(device._h, ctypes.byref(info), None, 0, big.ctypes.data_as(ctypes.c_void_p)))
    assert info.num_triangles == len(tris), form
    assert np.array_equal(big[:info.num_big], lc.big_triangles(tris)), (form, info.num_big)
    assert (3 if info.num_big >= 2 and lc.is_quads(tris[big[:info.num_big]]) else 0) == form.quads, form


@pytest.mark.parametrize("form", lc.FORMS, ids=[f.name for f in lc.FORMS])
def test_every_kind_under_the_form(device, form):
    scene4 = edge_scene(form.scene)[1]
    kinds = [k for f, k in lc.CELLS if f is form]
    assert len(kinds) >= 20
    slots = lc.slots()
    sky = Environment(env_map(lc.ENV_MAP))
    b = None
    try:
        with options(device, QUAD_FILTER=form.quad, ACCEL=form.accel):
            for kind in (k for k in kinds if not k.list):
                what = "%s %s" % (form.name, kind.name)
                want_fb, want_rad = lc.wanted(kind, form.scene)
                fb, ws = _render(device, kind, scene4, sky)
                assert_fb_equal(ws, want_rad, what + ": radiance before the fold")
                assert_fb_equal(fb, want_fb, what)
            b = PixelBuffers(device, scene4, lc.W, lc.H, frames=lc.FRAMES)
            for kind in (k for k in kinds if k.list):
                _run_list(device, b, form.scene, lc.W, lc.H, slots, lc.FRAMES, lc.K, lc.B, lc.R, lc.CAP, kind.mis, kind.power,
                          "%s %s" % (form.name, kind.name), candidates=lc.M if kind.ris else 0)
            if form.search == "lbvh":
                _assert_lbvh(device, form, scene4[0])
    finally:
        if b is not None:
            b.release()
        sky.release()
