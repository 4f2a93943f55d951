"""ctypes binding of tests/camera_oracle.c: the CPU oracle seen from any camera.  TEST INFRASTRUCTURE.

``python -B tests/camera_oracle.py build`` (what ``__graft_entry__.build()`` runs) builds the library of all three oracle
restatements, tests/oracles.py's.
"""
from __future__ import annotations

import os
import sys

import numpy as np

from oracles import build, cam10, lib, ptr


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


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
