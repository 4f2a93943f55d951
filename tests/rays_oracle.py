"""Builds, loads and binds tests/libtest_rays_oracle.so: the sample start of pt_radiance_rays (include/pt_shim.h) restated on the CPU
(tests/rays_oracles.c) -- ``orays_generate_ray``, getRay of a record of a ray table with no draw, in place of ``ocam_generate_ray`` under
the direct, indirect, MIS, power and roulette restatements, which are included as they are.  A library of its own, so that the other
oracle libraries stay as they are.  TEST INFRASTRUCTURE.

Inside ``with rays_oracle.rays(R, first_ray):`` the estimators' bindings go to this library with the table set:
``roulette_oracle.samples(tris, mats, W=first_ray + n, H=1, gid, frame, ...)`` is the sample of ray ``gid - first_ray``, and
``workspace`` / ``moments`` below put a whole call together.  The table is one file-scope value of the library: set before a call,
only read by its worker threads; blocks do not nest and are not entered from two threads at once.

``__graft_entry__.build()`` builds it (``python -B tests/rays_oracle.py build``); ``lib()`` builds it again when it is missing or older
than one of its sources.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np

import direct_oracle
import indirect_oracle
import mis_oracle
import moments_oracle
import oracles
import power_oracle
import roulette_oracle
from oracles import CFLAGS, I, I64, V, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtest_rays_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("rays_oracles.c", "camera_oracle.c", "direct_oracle.c", "indirect_oracle.c", "mis_oracle.c",
                                          "power_oracle.c", "roulette_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]
# the bindings whose calls a ``rays`` block redirects: each reaches its library through a module-level ``lib``
_BINDINGS = (direct_oracle, indirect_oracle, mis_oracle, power_oracle, roulette_oracle)

_SIGNATURES = {"orays_set": (I, [V, I64, I64])}


def build() -> str:
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
        sigs = dict(_SIGNATURES)
        for m in (power_oracle, roulette_oracle):
            sigs.update(m._SIGNATURES)
        # of libtest_oracles.so's entry points, those this library has too
        sigs.update({k: v for k, v in oracles._SIGNATURES.items() if hasattr(L, k)})
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def records(rays) -> np.ndarray:
    """pt_ray records (RAY_DTYPE or [n, 8] float32) as float32 [n, 8], contiguous"""
    return np.ascontiguousarray(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8))


@contextlib.contextmanager
def rays(R, first_ray=0):
    """inside the block, the estimators' bindings start pixel ``gid`` of a ``first_ray + len(R)`` x 1 image at record ``gid - first_ray``"""
    L = lib()
    r8 = records(R)
    if L.orays_set(ptr(r8) if len(r8) else None, len(r8), int(first_ray)) != 0:
        raise ValueError("ray ids past 2^31 - 1: %d rays from %d" % (len(r8), first_ray))
    saved = [(m, m.lib) for m in _BINDINGS]
    for m in _BINDINGS:
        m.lib = lib
    try:
        yield L
    finally:
        for m, f in saved:
            m.lib = f
        L.orays_set(None, 0, 0)


def workspace(tris, mats, R, samples, K, B, rr=(roulette_oracle.NEVER, 1.0), *, sample_begin=0, first_ray=0, mis=False, power=False,
              lights=None):
    """float32 [samples, n, 3]: what pt_radiance_rays leaves in a workspace that holds the whole call -- pt_render_indirect_rr's samples
    for an image of first_ray + n x 1 pixels whose pixel id starts at R[id - first_ray]"""
    r8 = records(R)
    n = len(r8)
    gid = np.tile(np.arange(first_ray, first_ray + n, dtype=np.int64), samples).astype(np.int32)
    frame = np.repeat(np.arange(sample_begin, sample_begin + samples, dtype=np.int64), n).astype(np.int32)
    if n == 0 or samples == 0:
        return np.zeros((samples, n, 3), np.float32)
    with rays(r8, first_ray):
        rad = roulette_oracle.samples(tris, mats, first_ray + n, 1, gid, frame, K, B, rr[0], rr[1], mis=mis, power=power, lights=lights)[0]
    return rad.reshape(samples, n, 3)


def moments(ws, start=None) -> np.ndarray:
    """the records pt_radiance_rays leaves in `moments` for that workspace (reset, or going on from ``start``)"""
    return moments_oracle.accumulate(ws, start)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
