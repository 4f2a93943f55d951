"""Every lit kernel once: the table of tests/test_gpu_lit_cells.py -- the 21 kinds of lit render under the 11 forms of the search, 231
cells, one kernel instantiation each -- and what the restatements say of every cell.  tests/test_lit_cells_cpu.py proves from this
table alone that each form's scene reaches its form.  TEST INFRASTRUCTURE.

A kind is what an entry point renders: direct illumination with the uniform or the power choice; indirect illumination, the roulette
(pt_render_indirect_rr) and the pixel list (pt_render_indirect_pixels), each for the four estimators (mis, power); resampled light
sampling with M = 8 candidates (direct, the roulette and the list kind by power, plain and MIS); environment lighting under a 16 x 16
map of distinct texels with one environment sample (direct, and the roulette kind by power with MIS) -- the 21 values that
ptk_lit_kind_valid accepts.  A form is what the search of a scene is: the LBVH, the table in LDS (at most 256 triangles) or the tiled
table; over packed quads, independent triangles with the short reciprocal (every |e1|_1 |e2|_1 <= PT_DET_BOUND_MAX = 2e19), or
unbounded ones.  Eight forms' scenes are scenes.direct_scaled's: 1, 10 and 15 nested Cornell boxes (36, 360 and 540 triangles) times
2^0, and times 2^30 for three unbounded forms: the largest |e1|_1 |e2|_1 of the box is 62.58, times 2^60 it is 7.2e19 (2^58 leaves
1.8e19, still bounded).  At that scale the reference's ray generator (eye + 4 dir, then - eye) rounds every primary direction away:
every sample of those cells is the background, in the restatements and on the device alike.  The cells of those three forms --
lbvh_unbounded, lds_unbounded, tiled_unbounded -- show that the unbounded kernels are launched, run and write the right records, not
what they compute.  The cells of lds_slab, tiled_slab and lbvh_slab (SHADING_UNBOUNDED) show what they compute: scenes.slab's 1, 10 and
15 boxes at unit scale beside one huge triangle under them, which alone lifts the scene over the bound; half of the first hits are on
that triangle, a quarter on the boxes, light samples at its vertices are open and occluded, and no sample is non-finite.

Every cell renders 24 x 16 pixels x 2 frames, K = 2, B = 6 -- 768 items: 12 waves, 3 workgroups -- the roulette kinds with R = 1 and a
cap of 0.25, so that roulette is played at every vertex, the list kinds a scattered list of 101 pixels at mixed frames."""
from __future__ import annotations

import collections

import numpy as np

import direct_oracle as do
import env_oracle as eo
import indirect_oracle as io
import mis_oracle as mo
import power_oracle as po
import ris_oracle as rs
import roulette_oracle as ro
from env_scenes import env_map
from scenes import edge_scene

W, H, FRAMES, K, B, R, CAP, LISTED = 24, 16, 2, 2, 6, 1, 0.25, 101
M, KE, ENV_MAP = 8, 1, "gradient:16"   # the RIS kinds' candidates; the env kinds' samples and map: a distinct value per texel, none of them 0.45
LDS_TRI_MAX, BVH_AUTO_MIN, DET_BOUND_MAX = 256, 512, np.float32(2.0e19)   # csrc/pt_kernels.h: PT_LDS_TRI_MAX, PT_BVH_AUTO_MIN, PT_DET_BOUND_MAX
BVH_BIG_DIV, BVH_BIG_MAX = np.float32(16.0), 64                          # csrc/pt_bvh.hip, csrc/pt_kernels.h

Kind = collections.namedtuple("Kind", "name indirect mis power rr list ris env", defaults=(False, False))
_ESTIMATORS = (("", False, False), ("_mis", True, False), ("_power", False, True), ("_mis_power", True, True))
KINDS = (Kind("direct", False, False, False, False, False), Kind("direct_power", False, False, True, False, False)) + \
    tuple(Kind(base + est, True, mis, power, rr, lst) for base, rr, lst in (("indirect", False, False), ("rr", True, False), ("list", True, True))
          for est, mis, power in _ESTIMATORS) + \
    (Kind("ris_direct", False, False, True, False, False, ris=True),) + \
    tuple(Kind("ris_" + base + est, True, mis, True, True, lst, ris=True) for base, lst in (("rr", False), ("list", True))
          for est, mis in (("", False), ("_mis", True))) + \
    (Kind("env_direct", False, False, True, False, False, env=True), Kind("env_rr_mis", True, True, True, True, False, env=True))
LIT_KIND_INDICES = 128   # csrc/pt_kernels.h: PT_LIT_KIND_INDICES


def kind_valid(k) -> bool:
    """ptk_lit_kind_valid (csrc/pt_kernels.h), restated"""
    return (not k.list or k.rr) and (not k.rr or k.indirect) and (not k.mis or k.indirect) and \
        (not k.ris or (k.power and k.rr == k.indirect)) and \
        (not k.env or (k.power and not k.ris and not k.list and k.rr == k.indirect and k.mis == k.indirect))


def kind_index(k) -> int:
    """ptk_lit_kind_index, restated"""
    return k.indirect | k.mis << 1 | k.power << 2 | k.rr << 3 | k.list << 4 | k.ris << 5 | k.env << 6

# search: "lbvh", "lds" or "tiled"; quads: 3 = the packed shared-u filter over the searched table, 0 = independent triangles;
# bounded: the short exact reciprocal.  quad / accel: PT_OPT_QUAD_FILTER / PT_OPT_ACCEL of the cell's renders
Form = collections.namedtuple("Form", "name scene quad accel search bounded quads")
FORMS = (
    # 36 triangles forced onto the LBVH: all of them are longer than 1/16 of the scene, so all 36 are the big table, which is quads
    Form("lbvh_quads", "scaled:1,0", 0, 2, "lbvh", True, 3),
    # 540 triangles take the LBVH by themselves; 520 of them are big, more than the table holds: the big table is empty
    Form("lbvh", "scaled:15,0", 0, 0, "lbvh", True, 0),
    Form("lbvh_unbounded", "scaled:15,30", 0, 0, "lbvh", False, 0),
    Form("lds_quads", "scaled:1,0", 0, 1, "lds", True, 3),
    Form("lds", "scaled:1,0", 1, 1, "lds", True, 0),
    Form("lds_unbounded", "scaled:1,30", 0, 1, "lds", False, 0),
    Form("tiled", "scaled:10,0", 0, 1, "tiled", True, 0),
    Form("tiled_unbounded", "scaled:10,30", 0, 1, "tiled", False, 0),
    # scenes.slab: the boxes at unit scale and one huge triangle that alone lifts the scene over the bound -- unbounded forms that shade.
    # At 15 copies the slab is the one triangle longer than 1/16 of the scene: a big table of one
    Form("lds_slab", "slab:1", 0, 1, "lds", False, 0),
    Form("tiled_slab", "slab:10", 0, 1, "tiled", False, 0),
    Form("lbvh_slab", "slab:15", 0, 0, "lbvh", False, 0),
)
SHADING_UNBOUNDED = ("lds_slab", "tiled_slab", "lbvh_slab")
# cells left out by name, with the reason: (form name, kind name).  None: all 231 are in the table
LEFT_OUT = ()
CELLS = tuple((f, k) for f in FORMS for k in KINDS if (f.name, k.name) not in LEFT_OUT)


# ---- what the table alone says of a scene (numpy, binary32 as the device computes it) -----------------------------------------------
def _corners(tris):
    return tuple(np.ascontiguousarray(tris[f][:, :3], np.float32) for f in ("p1", "p2", "p3"))


def det_bound(tris) -> np.float32:
    """max over the triangles of |e1|_1 |e2|_1 (pt_prep_kernel's word 0)"""
    p1, p2, p3 = _corners(tris)
    e1, e2 = np.abs(p2 - p1), np.abs(p3 - p1)
    return ((e1[:, 0] + e1[:, 1] + e1[:, 2]) * (e2[:, 0] + e2[:, 1] + e2[:, 2])).max()


def is_quads(tris) -> bool:
    """every pair (2k, 2k + 1) is (a, b, c), (c, d, a) with e2' == -e2 (pt_prep_kernel's words 1 and 3), an even number of them"""
    p1, _, p3 = _corners(tris)
    if len(p1) == 0 or len(p1) % 2:
        return False
    e2 = p3 - p1
    return bool((e2[1::2] == -e2[0::2]).all() and (p1[1::2] == p3[0::2]).all())


def big_triangles(tris) -> np.ndarray:
    """the indices the LBVH's builder keeps out of the hierarchy (pt_bvh.hip): boxes longer than 1/16 of the scene's longest side,
    ascending -- none when there are more than the table holds"""
    p1, p2, p3 = _corners(tris)
    lo, hi = np.minimum(np.minimum(p1, p2), p3), np.maximum(np.maximum(p1, p2), p3)
    thr = (hi.max(axis=0) - lo.min(axis=0)).max() / BVH_BIG_DIV
    big = np.flatnonzero((hi - lo).max(axis=1) > thr)
    return big if len(big) <= BVH_BIG_MAX else big[:0]


def form_of(tris, quad, accel):
    """(search, bounded, quads) as pt_shim.hip's prepare_search and the launchers decide them for a scene under the two options"""
    n = len(tris)
    bounded = bool(det_bound(tris) <= DET_BOUND_MAX)
    if n >= 2 and (accel == 2 or (accel == 0 and n >= BVH_AUTO_MIN)):
        big = big_triangles(tris)
        table_quads = len(big) >= 2 and bounded and is_quads(tris[big])
        return "lbvh", bounded, 3 if table_quads and quad in (0, 4) else 0
    if n <= LDS_TRI_MAX:
        return "lds", bounded, 3 if bounded and is_quads(tris) and quad in (0, 4) else 0
    return "tiled", bounded, 0   # (the tiled table has no packed form)


# ---- what the restatements say of a cell ----------------------------------------------------------------------------------------------
def _want(kind_name, scene):
    k = {k.name: k for k in KINDS}[kind_name]
    tris, mats, lights, cam = edge_scene(scene)[1]
    gid, frame = do.sample_ids(W, H, FRAMES)
    kw = dict(lights=lights, cam=cam)
    if k.ris:
        rkw = dict(B=B, R=R, cap=CAP, mis=k.mis, **kw) if k.indirect else kw
        fb, rad = rs.render(tris, mats, W, H, 0, FRAMES, K, M, **rkw), rs.samples(tris, mats, W, H, gid, frame, K, M, **rkw)
    elif k.env:
        ekw = dict(B=B, R=R, cap=CAP, **kw) if k.indirect else kw
        t = env_map(ENV_MAP)
        fb, rad = eo.render(tris, mats, t, W, H, 0, FRAMES, K, KE, **ekw), eo.samples(tris, mats, t, W, H, gid, frame, K, KE, **ekw)
    elif k.rr:
        fb = ro.render(tris, mats, W, H, 0, FRAMES, K, B, R, CAP, mis=k.mis, power=k.power, **kw)
        rad = ro.samples(tris, mats, W, H, gid, frame, K, B, R, CAP, mis=k.mis, power=k.power, **kw)[0]
    elif k.power:
        mode = po.MIS if k.mis else po.INDIRECT if k.indirect else po.DIRECT
        fb, rad = po.render(mode, tris, mats, W, H, 0, FRAMES, K, B, **kw), po.samples(mode, tris, mats, W, H, gid, frame, K, B, **kw)
    elif not k.indirect:
        fb, rad = do.render(tris, mats, W, H, 0, FRAMES, K, **kw), do.decisions(tris, mats, W, H, gid, frame, K, **kw)[2]
    elif k.mis:
        fb, rad = mo.render(tris, mats, W, H, 0, FRAMES, K, B, **kw), mo.samples(tris, mats, W, H, gid, frame, K, B, **kw)[0]
    else:
        fb, rad = io.render(tris, mats, W, H, 0, FRAMES, K, B, **kw), io.samples(tris, mats, W, H, gid, frame, K, B, **kw)[0]
    return fb, rad.reshape(FRAMES, -1, 3)


def wanted(kind, scene):
    """the restatement's (framebuffer, radiance [FRAMES, pixels, 3]) of a kind that is no list kind on a scene: computed once, shared,
    read-only.  (A list kind's is adaptive_support._expect of ``slots()``.)"""
    assert not kind.list
    return do.once(_want, kind.name, scene)


def slots():
    """the list of the list kinds: LISTED of the W x H pixels in no order, each at a frame of its own in [0, 6], some at 0"""
    from adaptive_support import _scattered

    return _scattered(np.random.default_rng(LISTED), W * H, LISTED)
