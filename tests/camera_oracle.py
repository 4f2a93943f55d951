"""ctypes binding of tests/camera_oracle.c: the CPU oracle seen from any camera.  TEST INFRASTRUCTURE (the library: tests/oracles.py).
"""
from __future__ import annotations

import os

import numpy as np

from oracles import I, I64, V, cam10, declare, lib, ptr

declare({
    "ocam_derive": (I, [V, V]),
    "ocam_render": (I, [V, I, V, I, V, I, I, I, I, I, I64, I64, I, V, V]),
})


def derive(eye, center, up, fov_y_deg):
    """ocam_derive: float32[16] of derived values, or None for a camera the contract rejects."""
    cin = np.array(list(eye) + list(center) + list(up) + [fov_y_deg], np.float32)
    out = np.zeros(16, np.float32)
    rc = lib().ocam_derive(ptr(cin), ptr(out))
    return None if rc != 0 else out


def render(tris, mats, W, H, frames, cam, *, frame_begin=0, max_bounces=16, fb=None, gid_begin=0, gid_count=None,
           nthreads=None, want_stats=False):
    """ptoracle.render seen from ``cam`` (a Camera).  Returns the (H*W, 4) float32 framebuffer and, if asked, the tallies."""
    from oracle import ptoracle

    tris = np.ascontiguousarray(tris)
    mats = np.ascontiguousarray(mats)
    if fb is None:
        fb = np.zeros((H * W, 4), np.float32)
    assert fb.dtype == np.float32 and fb.size == W * H * 4 and fb.flags.c_contiguous
    if gid_count is None:
        gid_count = W * H - gid_begin
    if nthreads is None:
        nthreads = min(os.cpu_count() or 1, 16)
    st = np.zeros(len(ptoracle.STATS_FIELDS), np.uint64)
    c = cam10(cam)
    rc = lib().ocam_render(ptr(tris), len(tris), ptr(mats), len(mats), ptr(fb), W, H, frame_begin, frames, max_bounces,
                           gid_begin, gid_count, nthreads, ptr(st), ptr(c))
    if rc != 0:
        raise ValueError("ocam_render rejected the arguments (rc=%d)" % rc)
    if want_stats:
        return fb, dict(zip(ptoracle.STATS_FIELDS, (int(v) for v in st)))
    return fb
