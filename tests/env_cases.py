"""The single table of inputs of the environment-lighting tests: tests/test_gpu_env.py renders every case on the device and compares
it with the restatement, tests/test_env_cpu.py proves on the CPU that each case reaches the edge it is there for.  TEST
INFRASTRUCTURE."""
from __future__ import annotations

import collections

NEVER = 65535   # a first_bounce no path reaches: no roulette

# scene, map: names of env_scenes.env_scene / env_map.  B None: pt_render_direct_env, otherwise pt_render_indirect_env with the roulette
# (R, cap).  search: (PT_OPT_QUAD_FILTER, PT_OPT_ACCEL) -- ACCEL 0 takes brute force below 512 triangles (the table in LDS up to 256, tiled
# above) and the LBVH from 512 on; 1 forces brute force, 2 the LBVH.  stripes: (stripe_rows, n_ranks) rendered rank by rank.
# chunk: the workspace's frames (None: all of the call's).  nl0: render with num_lights = 0 (every emitter buffer NULL)
Case = collections.namedtuple("Case", "id scene map W H frames K Ke B R cap search frame_begin stripes chunk nl0")


def case(id, scene, map, W, H, frames, K=1, Ke=1, B=None, R=NEVER, cap=1.0, search=(1, 0), frame_begin=0, stripes=None, chunk=None, nl0=False):
    return Case(id, scene, map, W, H, frames, K, Ke, B, R, cap, search, frame_begin, stripes, chunk, nl0)


def _both(id, *a, B=4, **kw):
    """the case through both estimators"""
    return [case(id + "-direct", *a, **kw), case(id + "-indirect", *a, B=B, **kw)]


CASES = (
    # the four scenes, both estimators; image sizes of 1, 15, 65 and 40 x 24 pixels; the three searches; the quad filter on and off
    _both("open-sun-40x24", "open", "sun", 40, 24, 2, Ke=1)
    + _both("open-gradient-1px", "open", "gradient:16", 1, 1, 3, Ke=3)
    + _both("panel-sun-15px", "open_panel", "sun", 5, 3, 2, Ke=3, search=(0, 0))
    + _both("panel-gradient-65px", "open_panel", "gradient:16", 13, 5, 2, Ke=1, search=(4, 1))
    + _both("many-sun-lbvh", "many_open", "sun", 40, 24, 1, Ke=1)
    + _both("many-gradient-lbvh-noquad", "many_open", "gradient:16", 13, 5, 2, Ke=3, search=(0, 0))
    + _both("tiled-sun", "many_tiled_open", "sun", 40, 24, 1, Ke=1)
    + _both("tiled-gradient-noquad", "many_tiled_open", "gradient:2", 5, 3, 2, Ke=3, search=(0, 0))
    + _both("floor-grey", "floor", "grey:1", 40, 24, 2, Ke=1)
    + _both("open-lbvh-forced", "open", "sun", 13, 5, 2, Ke=1, search=(1, 2))
    # Ke = 0, 1, 3, 256
    + _both("panel-Ke0", "open_panel", "gradient:16", 40, 24, 2, Ke=0)
    + _both("panel-Ke256", "open_panel", "sun", 5, 3, 1, Ke=256)
    + _both("many-Ke256-lbvh", "many_open", "sun", 5, 3, 1, Ke=256, B=2)
    # num_lights = 0 on a scene that has emitters
    + _both("panel-nl0", "open_panel", "sun", 40, 24, 2, Ke=1, nl0=True)
    + _both("many-nl0-lbvh", "many_open", "sun", 13, 5, 1, Ke=3, nl0=True)
    # depth and roulette
    + [case("panel-B1", "open_panel", "sun", 40, 24, 2, Ke=1, B=1),
       case("panel-B16", "open_panel", "sun", 40, 24, 2, Ke=1, B=16),
       case("panel-B16-rr", "open_panel", "sun", 40, 24, 2, Ke=1, B=16, R=1, cap=0.95),
       case("many-B16-rr-lbvh", "many_open", "gradient:16", 40, 24, 1, Ke=1, B=16, R=1, cap=0.95),
       case("tiled-B16-rr", "many_tiled_open", "sun", 13, 5, 1, Ke=1, B=16, R=1, cap=0.95),
       case("open-B4-rr-Ke0", "open", "gradient:16", 40, 24, 2, Ke=0, B=4, R=1, cap=0.95)]
    # K > 1 beside Ke > 1
    + _both("panel-K3-Ke3", "open_panel", "sun", 13, 5, 2, K=3, Ke=3)
    # three-rank stripes, two chunks through a workspace of one frame, a later first frame, a camera below the horizon
    + _both("panel-stripes", "open_panel", "sun", 40, 24, 2, Ke=1, stripes=(5, 3))
    + _both("many-stripes-lbvh", "many_open", "sun", 40, 24, 1, Ke=1, stripes=(5, 3))
    + _both("panel-chunks", "open_panel", "gradient:16", 40, 24, 2, Ke=1, chunk=1)
    + _both("many-chunks-lbvh", "many_open", "sun", 13, 5, 2, Ke=1, chunk=1)
    + _both("panel-frame7", "open_panel", "sun", 40, 24, 2, Ke=1, frame_begin=7)
    + _both("below-horizon", "below", "gradient:16", 40, 24, 2, Ke=3)
    # the edges: a map with NaN, negative, infinite and -0 texels; an all-zero map sampled; N = 1; N = 2048 looked up; a glossy room whose
    # paths go NaN; a material of neither type; no triangle at all
    + _both("bad-map", "open_panel", "bad:16", 40, 24, 2, Ke=3)
    + _both("zero-map", "open_panel", "zero:4", 40, 24, 2, Ke=3)
    + _both("N1", "open_panel", "gradient:1", 40, 24, 2, Ke=3)
    + _both("glossy-nan", "glossy", "sun", 40, 24, 2, Ke=1, B=8)
    + _both("glossy-nan-lbvh", "glossy", "gradient:16", 40, 24, 1, Ke=1, B=8, search=(1, 2))
    + _both("other-type", "other_type", "sun", 40, 24, 1, Ke=3)
    + _both("empty-scene", "empty", "gradient:16", 40, 24, 2, Ke=1)
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
