"""The inputs of tests/test_gpu_ris.py and what the restatement (tests/ris_oracle.c) says of them: one table, so that
tests/test_ris_cpu.py proves on exactly the scenes and sizes the device renders that every edge of the resampling is reached.
TEST INFRASTRUCTURE.

A case is (scene, W, H, frames, K, M, B, R, cap, mis): a name of ris_scenes.ris_scene, the image, the frames, K light samples of M
candidates, and for the indirect form the depth B (None: pt_render_direct_ris), the roulette (R, cap) and mis."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import direct_oracle as do
import ris_oracle as rs
from ris_scenes import ris_scene

NEVER = rs.NEVER
OFF, SOFT, HARD = (NEVER, 1.0), (1, 0.95), (3, 0.5)          # the roulette settings: none (R >= B), and the two played
MS = (1, 2, 8, 32)
# images: 1, 15 and 65 pixels (partial waves; a refill run that does not fill) and 40 x 24 (15 waves)
ONE, FIFTEEN, SIXTYFIVE, BIG = (1, 1), (5, 3), (13, 5), (40, 24)


def _direct(scene, size, K, M, frames=1):
    return (scene, size[0], size[1], frames, K, M, None, NEVER, 1.0, False)


def _indirect(scene, size, K, M, B, rr, mis, frames=1):
    return (scene, size[0], size[1], frames, K, M, B, rr[0], rr[1], bool(mis))


# the room of 64 equal emitters through the brute-force kernels (PT_OPT_ACCEL 1)
DIRECT = [_direct("many", BIG, 1, 2), _direct("many", BIG, 1, 8), _direct("many", SIXTYFIVE, 4, 32), _direct("many", SIXTYFIVE, 4, 1),
          _direct("many", FIFTEEN, 4, 8), _direct("many", ONE, 1, 32), _direct("many", ONE, 4, 2)]
DEEP = _direct("many", FIFTEEN, 256, 32)                      # K = 256 with M = 32: 8191 uniforms per light sample loop of a pixel
INDIRECT = [_indirect("many", BIG, 1, 8, 8, OFF, False), _indirect("many", BIG, 1, 2, 8, SOFT, True), _indirect("many", BIG, 1, 32, 8, HARD, True),
            _indirect("many", BIG, 1, 8, 8, HARD, False), _indirect("many", SIXTYFIVE, 4, 2, 2, OFF, True), _indirect("many", SIXTYFIVE, 4, 8, 2, SOFT, False),
            _indirect("many", SIXTYFIVE, 1, 1, 8, HARD, True), _indirect("many", FIFTEEN, 4, 32, 8, SOFT, True), _indirect("many", FIFTEEN, 1, 2, 2, HARD, False),
            _indirect("many", ONE, 4, 8, 8, SOFT, True), _indirect("many", ONE, 1, 32, 2, OFF, False), _indirect("many", SIXTYFIVE, 4, 8, 1, OFF, True)]
# the tiled table (257 .. 511 triangles) and the LBVH (512 and more)
TILED = [_direct("many_tiled", SIXTYFIVE, 4, 8), _indirect("many_tiled", BIG, 1, 8, 8, HARD, True), _indirect("many_tiled", FIFTEEN, 4, 2, 2, SOFT, False)]
LBVH = [_direct("many_lbvh", BIG, 1, 8), _direct("many_lbvh", FIFTEEN, 4, 32), _indirect("many_lbvh", BIG, 1, 8, 8, HARD, True),
        _indirect("many_lbvh", SIXTYFIVE, 4, 32, 2, OFF, False), _indirect("many_lbvh", BIG, 1, 2, 8, SOFT, False), _indirect("many_lbvh", ONE, 4, 8, 8, SOFT, True)]
# every search option over the one scene: (PT_OPT_QUAD_FILTER, PT_OPT_ACCEL) -- the LBVH is forced on 100 triangles by ACCEL 2
SEARCH_CASES = [_direct("many", SIXTYFIVE, 4, 8), _indirect("many", SIXTYFIVE, 1, 8, 8, HARD, True)]
# the lists at the choice's edges, and light indices out of range (clamped)
LISTS = [_direct("edge_list", SIXTYFIVE, 4, 8), _indirect("edge_list", SIXTYFIVE, 1, 8, 4, SOFT, True), _direct("zero_list", FIFTEEN, 4, 8),
         _indirect("zero_list", FIFTEEN, 1, 2, 4, SOFT, True), _direct("out_of_range", SIXTYFIVE, 4, 8),
         _indirect("out_of_range", SIXTYFIVE, 1, 8, 4, HARD, True)]
# vertices within 0.02 of an emitter: kept candidates whose ray is open without a search (360 triangles: the tiled table)
NEAR = [_direct("scaled", SIXTYFIVE, 4, 8), _indirect("scaled", SIXTYFIVE, 1, 8, 4, SOFT, True)]
# the identity scenes of M = 1: direct against pt_render_direct_power, indirect against pt_render_indirect_rr with the table
IDENTITY = [_direct("cornell", BIG, 4, 1), _direct("unequal", BIG, 4, 1), _indirect("cornell", BIG, 1, 1, 8, HARD, True),
            _indirect("unequal", BIG, 1, 1, 8, SOFT, False), _indirect("cornell", SIXTYFIVE, 4, 1, 2, OFF, True)]
# B = 1 against the direct form at the same M
B_ONE = [(_indirect("many", SIXTYFIVE, 4, 8, 1, OFF, mis), _direct("many", SIXTYFIVE, 4, 8)) for mis in (False, True)]
# two frames in two chunks; three-rank stripes
CHUNKED = [_direct("many", SIXTYFIVE, 4, 8, frames=2), _indirect("many", SIXTYFIVE, 1, 8, 8, HARD, True, frames=2)]
STRIPED = _indirect("many", BIG, 1, 8, 8, SOFT, True)
STRIPES = dict(stripe_rows=5, n_ranks=3)
# the adaptive render and the Python renderers
ADAPTIVE = _indirect("many", (16, 16), 1, 8, 4, SOFT, True)
PYTHON = [_direct("many", SIXTYFIVE, 4, 8), _indirect("many", SIXTYFIVE, 1, 8, 8, HARD, True)]

# the resampling's edges: name -> case.  tests/test_ris_cpu.py proves each is reached (on the device's own inputs: each is in a list above)
EDGES = {
    "keeps_first": INDIRECT[0],          # a light sample that keeps candidate 0 although later ones had s > 0
    "keeps_last": INDIRECT[0],           # ... that keeps candidate M - 1
    "replaces": INDIRECT[0],             # ... in which a later candidate replaced an earlier one
    "none_kept": DIRECT[1],              # have = false with M > 1: no ray
    "unsearched": NEAR[0],              # a kept candidate with tl <= 0 (a vertex within 0.02 of an emitter): open, no search
    "occluded": INDIRECT[2],             # a kept candidate that ends occluded
    "open": INDIRECT[2],                 # ... and one that ends open
    "weighted": INDIRECT[2],             # with MIS: a kept candidate that carries the balance factor
    "last_vertex": INDIRECT[2],          # ... one at the path's last vertex (not weighted)
    "back_side": INDIRECT[2],            # ... one seen from behind, sl <= 0 (not weighted)
    "zero_total": LISTS[3],              # a table of total 0: the uniforms are drawn, nothing contributes
    "edge_list": LISTS[1],               # q = 0 walls, the emitter of no area, duplicates
}


def is_direct(case):
    return case[6] is None


def _want(name, W, H, frames, K, M, B, R, cap, mis, frame_begin=0, **stripes):
    tris, mats, lights, cam = ris_scene(name)
    gid, frame = do.sample_ids(W, H, frames, **stripes)
    kw = dict(B=B, R=R, cap=cap, mis=mis, lights=lights, cam=cam)
    return (rs.render(tris, mats, W, H, frame_begin, frames, K, M, **kw, **stripes),
            rs.samples(tris, mats, W, H, gid, frame + frame_begin, K, M, **kw).reshape(frames, -1, 3))


def wanted(case, **kw):
    """the restatement's (framebuffer, radiance [frames, local pixels, 3]) of a case: computed once, shared, read-only"""
    return do.once(_want, *case, **kw)


def prefetch(cases):
    """``wanted`` of many cases on threads: the library holds no state"""
    rs.lib()
    with ThreadPoolExecutor(rs.THREADS) as ex:
        list(ex.map(wanted, cases))


def details(case):
    """(radiance, the per-light-sample account) of every sample of a case (ris_oracle.samples with details)"""
    name, W, H, frames, K, M, B, R, cap, mis = case
    tris, mats, lights, cam = ris_scene(name)
    gid, frame = do.sample_ids(W, H, frames)
    return rs.samples(tris, mats, W, H, gid, frame, K, M, B=B, R=R, cap=cap, mis=mis, lights=lights, cam=cam, details=True)


def all_cases():
    out = DIRECT + [DEEP] + INDIRECT + TILED + LBVH + LISTS + NEAR + IDENTITY + [c for pair in B_ONE for c in pair] + CHUNKED
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq
