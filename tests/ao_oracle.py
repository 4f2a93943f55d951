"""ctypes binding of tests/ao_oracle.c: the CPU oracle's ambient occlusion -- the counts {open, hits} of pt_render_ao, and the
per-ray decisions behind them.  TEST INFRASTRUCTURE.

Compiled on demand with oracle/Makefile's flags, as tests/camera_oracle.py does.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libao_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("ao_oracle.c", "camera_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]


def build() -> str:
    from camera_oracle import CFLAGS

    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc] + CFLAGS + ["-shared", "-o", LIB_PATH, _SRCS[0], "-lm", "-lpthread"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(f) for f in _SRCS):
            build()
        L = ctypes.CDLL(LIB_PATH)
        L.oao_render.restype = ctypes.c_int
        L.oao_render.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_float, ctypes.c_void_p]
        L.oao_decisions.restype = None
        L.oao_decisions.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _cam10(cam):
    if cam is None:
        return None
    return np.array(list(cam.eye) + list(cam.center) + list(cam.up) + [cam.fov_y_deg], np.float32)


def counts(tris, W, H, frame_begin, frame_count, K, radius, cam=None, stripe_rows=1, n_ranks=1, rank=0, start=None):
    """uint32 [local rows, W, 2] {open, hits} over frames [frame_begin, frame_begin + frame_count), added to `start` (or zeros);
    None when the camera is rejected.  cam: a Camera (None = the reference's)."""
    tris = np.ascontiguousarray(tris)
    rows = sum(1 for r in range(H) if (r // stripe_rows) % n_ranks == rank)
    out = np.zeros((rows, W, 2), np.uint32) if start is None else np.array(start, np.uint32).reshape(rows, W, 2).copy()
    c = _cam10(cam)
    rc = lib().oao_render(_ptr(tris) if len(tris) else None, len(tris), _ptr(c) if c is not None else None, W, H, stripe_rows, n_ranks,
                          rank, frame_begin, frame_count, K, float(radius), _ptr(out))
    return None if rc != 0 else out


def decisions(tris, W, H, gid, frame, K, radius):
    """Per sample (gid[i], frame[i]) of the reference's camera: hit (uint8 [n]) and open (uint8 [n, K], 1 = the ray is open)."""
    tris = np.ascontiguousarray(tris)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    hit = np.zeros(len(gid), np.uint8)
    open_k = np.zeros((len(gid), K), np.uint8)
    lib().oao_decisions(_ptr(tris), len(tris), W, H, _ptr(gid), _ptr(frame), len(gid), K, float(radius), _ptr(hit), _ptr(open_k))
    return hit, open_k
