"""Builds and loads tests/libtest_oracles.so: the CPU oracle (oracle/pt_oracle.c) with every restatement of it -- the camera, query and
ambient-occlusion ones, direct and indirect illumination, multiple importance sampling, the primary rays' accepted sets and the windowed render of very large images -- as one
translation unit, tests/oracles.c.  TEST INFRASTRUCTURE.

``__graft_entry__.build()`` builds it (``python -B tests/oracles.py build``); ``lib()`` builds it again when it is missing or older
than one of its sources, as ``ptoracle.lib()`` does.  The bindings are tests/camera_oracle.py, query_oracle.py, ao_oracle.py,
direct_oracle.py, indirect_oracle.py, mis_oracle.py, primary_accept.py and extent_oracle.py: each declares its entry points here (``declare``).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtest_oracles.so")
_SRCS = [os.path.join(_HERE, f) for f in ("oracles.c", "camera_oracle.c", "query_oracle.c", "ao_oracle.c", "direct_oracle.c",
                                          "indirect_oracle.c", "mis_oracle.c", "primary_accept.c", "extent_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]
# a copy of oracle/Makefile's CFLAGS: strict IEEE, no contraction, no fast-math
CFLAGS = ["-O2", "-fPIC", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-function", "-ffp-contract=off", "-fno-fast-math",
          "-fno-math-errno", "-pthread"]

V, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_SIGNATURES = {}   # entry point -> (restype, argtypes): what the binding modules have declared


def build() -> str:
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc] + CFLAGS + ["-shared", "-o", LIB_PATH, _SRCS[0], "-lm", "-lpthread"])
    return LIB_PATH


_lib = None


def _bind(L, signatures):
    for name, (res, args) in signatures.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args


def declare(signatures):
    """a binding module's entry points, name -> (restype, argtypes): set on the library when ``lib()`` loads it, or now if it has"""
    _SIGNATURES.update(signatures)
    if _lib is not None:
        _bind(_lib, signatures)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(f) for f in _SRCS):
            build()
        L = ctypes.CDLL(LIB_PATH)
        _bind(L, _SIGNATURES)
        _lib = L
    return _lib


def ptr(a):
    """the data of an array as void*; None (no camera) stays NULL"""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def cam10(cam):
    """eye, center, up, fov_y_deg of a Camera (or of any object with those attributes) as float32[10]; None stays None."""
    if cam is None:
        return None
    return np.array(list(cam.eye) + list(cam.center) + list(cam.up) + [cam.fov_y_deg], np.float32)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
