"""Builds, loads and binds tests/libtest_lens_oracle.so: the thin lens of include/pt_shim.h (pt_camera) restated on the CPU
(tests/lens_oracles.c) -- ``olens_generate_ray`` in place of ``ocam_generate_ray`` under the ambient-occlusion, direct, indirect, MIS,
power, roulette, RIS and environment restatements, which are included as they are.  A library of its own, so that the other oracle
libraries stay as they are.  TEST INFRASTRUCTURE.

The estimators' bindings are the ones that exist (``ao_oracle``, ``direct_oracle``, ``indirect_oracle``, ``mis_oracle``, ``power_oracle``,
``roulette_oracle``, ``ris_oracle``, ``env_oracle``): inside ``with lens_oracle.lens(R, F):`` their calls go to this library with the lens
set, e.g. ``roulette_oracle.samples(...)`` is the lens render's samples.  The lens is one file-scope value of the library: set before
a call, only read by its worker threads; blocks do not nest and are not entered from two threads at once.

``__graft_entry__.build()`` builds it (``python -B tests/lens_oracle.py build``); ``lib()`` builds it again when it is missing or older
than one of its sources.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np

import ao_oracle
import direct_oracle
import env_oracle
import indirect_oracle
import mis_oracle
import oracles
import power_oracle
import ris_oracle
import roulette_oracle
from oracles import CFLAGS, F, I, I64, V, cam10, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtest_lens_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("lens_oracles.c", "camera_oracle.c", "ao_oracle.c", "direct_oracle.c", "indirect_oracle.c",
                                          "mis_oracle.c", "power_oracle.c", "roulette_oracle.c", "ris_oracle.c", "env_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]
# the bindings whose calls a ``lens`` block redirects: each reaches its library through a module-level ``lib``
_BINDINGS = (ao_oracle, direct_oracle, indirect_oracle, mis_oracle, power_oracle, roulette_oracle, ris_oracle, env_oracle)

_SIGNATURES = {
    "olens_set": (I, [F, F]),
    "olens_camera_rays": (I, [V, I, I, I, V]),
    "olens_rays": (None, [V, I, I, V, V, I64, V]),
}


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
        for m in (power_oracle, roulette_oracle, ris_oracle, env_oracle):
            sigs.update(m._SIGNATURES)
        # of libtest_oracles.so's entry points, those this library has too (the query, accepted-set and extent restatements are not here)
        sigs.update({k: v for k, v in oracles._SIGNATURES.items() if hasattr(L, k)})
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


@contextlib.contextmanager
def lens(R, F):
    """inside the block, the estimators' bindings compute with the thin lens (R, F); (0, F) is the pinhole, through this library"""
    L = lib()
    if L.olens_set(float(R), float(F)) != 0:
        raise ValueError("a lens pt_camera_derive rejects: R = %r, F = %r" % (R, F))
    saved = [(m, m.lib) for m in _BINDINGS]
    for m in _BINDINGS:
        m.lib = lib
    try:
        yield L
    finally:
        for m, f in saved:
            m.lib = f
        L.olens_set(0.0, 0.0)


def lens_of(cam):
    """(R, F) of a Camera; (0, 0) for None"""
    return (0.0, 0.0) if cam is None else (cam.lens_radius, cam.focus_distance)


def camera_rays(cam, W, H, frame):
    """float32 [W * H, 8]: pt_camera_rays' records -- origin, 1e20, the direction getRay receives (normalised once), 0 -- for ``cam``
    with its lens; None when the camera is rejected"""
    out = np.zeros((W * H, 8), np.float32)
    with lens(*lens_of(cam)) as L:
        rc = L.olens_camera_rays(ptr(cam10(cam)), W, H, frame, ptr(out))
    return None if rc != 0 else out


def rays(cam, W, H, gid, frame, R=None, F=None):
    """(origin, direction) float32 [n, 3] of the samples (gid[i], frame[i]): the ray getRay returns, for ``cam`` with its lens or (R, F)"""
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    out = np.zeros((len(gid), 6), np.float32)
    rf = lens_of(cam) if R is None else (R, F)
    with lens(*rf) as L:
        L.olens_rays(ptr(cam10(cam)), W, H, ptr(gid), ptr(frame), len(gid), ptr(out))
    return out[:, :3].copy(), out[:, 3:].copy()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
