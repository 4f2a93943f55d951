"""ctypes binding of tests/camera_oracle.c: the CPU oracle seen from any camera.  TEST INFRASTRUCTURE.

Built beside the oracle by ``__graft_entry__.build()`` (``python -B tests/camera_oracle.py build``) with oracle/Makefile's
flags, and again on demand when the library is missing, as ``ptoracle.lib()`` does.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libcamera_oracle.so")
# oracle/Makefile's CFLAGS: strict IEEE, no contraction, no fast-math
CFLAGS = ["-O2", "-fPIC", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-function", "-ffp-contract=off", "-fno-fast-math",
          "-fno-math-errno", "-pthread"]


def build() -> str:
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc] + CFLAGS + ["-shared", "-o", LIB_PATH, os.path.join(_HERE, "camera_oracle.c"), "-lm", "-lpthread"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = ctypes.CDLL(LIB_PATH)
        L.ocam_derive.restype = ctypes.c_int
        L.ocam_derive.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.ocam_render.restype = ctypes.c_int
        L.ocam_render.argtypes = [
            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
        ]
        _lib = L
    return _lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _cam10(cam) -> np.ndarray:
    """eye, center, up, fov_y_deg of a Camera (or of any object with those attributes) as float32[10]."""
    return np.array(list(cam.eye) + list(cam.center) + list(cam.up) + [cam.fov_y_deg], np.float32)


def derive(eye, center, up, fov_y_deg):
    """ocam_derive: float32[16] of derived values, or None for a camera the contract rejects."""
    cin = np.array(list(eye) + list(center) + list(up) + [fov_y_deg], np.float32)
    out = np.zeros(16, np.float32)
    rc = lib().ocam_derive(_ptr(cin), _ptr(out))
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
    c = _cam10(cam)
    rc = lib().ocam_render(_ptr(tris), len(tris), _ptr(mats), len(mats), _ptr(fb), W, H, frame_begin, frames, max_bounces,
                           gid_begin, gid_count, nthreads, _ptr(st), _ptr(c))
    if rc != 0:
        raise ValueError("ocam_render rejected the arguments (rc=%d)" % rc)
    if want_stats:
        return fb, dict(zip(ptoracle.STATS_FIELDS, (int(v) for v in st)))
    return fb


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
