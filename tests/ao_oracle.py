"""ctypes binding of tests/ao_oracle.c: the CPU oracle's ambient occlusion -- the counts {open, hits} of pt_render_ao, and the
per-ray decisions behind them.  TEST INFRASTRUCTURE (the library: tests/oracles.py).
"""
from __future__ import annotations

import numpy as np

import direct_oracle
from oracles import F, I, I64, V, cam10, declare, lib, ptr

declare({
    "oao_render": (I, [V, I, V] + [I] * 8 + [F, V]),
    "oao_decisions": (None, [V, I, I, I, V, V, I64, I, F, V, V]),
})


def counts(tris, W, H, frame_begin, frame_count, K, radius, cam=None, stripe_rows=1, n_ranks=1, rank=0, start=None):
    """uint32 [local rows, W, 2] {open, hits} over frames [frame_begin, frame_begin + frame_count), added to `start` (or zeros);
    None when the camera is rejected.  cam: a Camera (None = the reference's)."""
    tris = np.ascontiguousarray(tris)
    rows = direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)
    out = np.zeros((rows, W, 2), np.uint32) if start is None else np.array(start, np.uint32).reshape(rows, W, 2).copy()
    c = cam10(cam)
    rc = lib().oao_render(ptr(tris) if len(tris) else None, len(tris), ptr(c), W, H, stripe_rows, n_ranks,
                          rank, frame_begin, frame_count, K, float(radius), ptr(out))
    return None if rc != 0 else out


def decisions(tris, W, H, gid, frame, K, radius):
    """Per sample (gid[i], frame[i]) of the reference's camera: hit (uint8 [n]) and open (uint8 [n, K], 1 = the ray is open)."""
    tris = np.ascontiguousarray(tris)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    hit = np.zeros(len(gid), np.uint8)
    open_k = np.zeros((len(gid), K), np.uint8)
    lib().oao_decisions(ptr(tris), len(tris), W, H, ptr(gid), ptr(frame), len(gid), K, float(radius), ptr(hit), ptr(open_k))
    return hit, open_k


# the unbounded scenes that shade (scenes.slab; tests/lit_cells.py has their forms): (search, scene, PT_OPT_ACCEL), and the render of
# tests/test_gpu_ao.py on them -- a radius no hit lies beyond, so that rays from the boxes reach the slab far out
SLAB_FORMS = (("lds", "slab:1", 1), ("tiled", "slab:10", 1), ("lbvh", "slab:15", 0))
SLAB_W, SLAB_H, SLAB_FRAMES, SLAB_K, SLAB_RADIUS = 24, 16, 2, 4, 1e20


def _slab_counts(scene):
    from scenes import edge_scene

    tris, _, _, cam = edge_scene(scene)[1]
    return (counts(tris, SLAB_W, SLAB_H, 0, SLAB_FRAMES, SLAB_K, SLAB_RADIUS, cam=cam),)


def slab_counts(scene):
    """the counts of the slab render of ``scene``: computed once, shared, read-only"""
    return direct_oracle.once(_slab_counts, scene)[0]
