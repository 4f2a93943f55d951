"""ctypes binding of tests/extent_oracle.c: the fused renderer's pixels at listed gids of an image too large to hold (the CPU oracle's
own sample and fold), with the rays it traced.  TEST INFRASTRUCTURE (the library: tests/oracles.py).
"""
from __future__ import annotations

import numpy as np

from oracle import ptoracle
from oracles import I, I64, V, declare, lib, ptr

declare({
    "oex_render_window": (I, [V, I, V, I, I, I, I, I, V, I64, V, V]),
})


def render_window(tris, mats, W, H, frames, gid, *, frame_begin=0, max_bounces=16, start=None):
    """(pixels float32 [n, 4], tallies dict): frames [frame_begin, frame_begin + frames) of the pixels ``gid`` (global indices, any
    order) of the W x H image folded into ``start`` ([n, 4]; None = zeros), and ptoracle's work tallies over them ("rays",
    "samples", ...) -- what ``ptoracle.render`` gives at those pixels, without its W x H framebuffer."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    g = np.ascontiguousarray(gid, np.int64)
    assert g.ndim == 1 and (not len(g) or (0 <= g.min() and g.max() < W * H)), "a gid outside the image"
    g = g.astype(np.int32)
    px = np.zeros((len(g), 4), np.float32) if start is None else np.array(start, np.float32).reshape(len(g), 4).copy()
    st = np.zeros(len(ptoracle.STATS_FIELDS), np.uint64)
    rc = lib().oex_render_window(ptr(tris) if len(tris) else None, len(tris), ptr(mats), W, H, frame_begin, frames, max_bounces,
                                 ptr(g), len(g), ptr(px), ptr(st))
    if rc != 0:
        raise ValueError("oex_render_window rejected the arguments")
    return px, dict(zip(ptoracle.STATS_FIELDS, (int(v) for v in st)))
