"""Builds, loads and binds tests/libtest_feature_oracle.so: the first-hit feature samples of pt_render_features restated on the CPU
(tests/feature_oracle.c, on tests/lens_oracles.c and through it on oracle/pt_oracle.c).  A library of its own, so that the other oracle
libraries stay as they are.  TEST INFRASTRUCTURE.

``__graft_entry__.build()`` builds it (``python -B tests/feature_oracle.py build``); ``lib()`` builds it again when it is missing or
older than one of its sources.
"""
from __future__ import annotations

import collections
import ctypes
import os
import subprocess
import sys

import numpy as np

import direct_oracle
from oracles import CFLAGS, F, I, V, cam10, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtest_feature_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("feature_oracle.c", "lens_oracles.c", "camera_oracle.c", "ao_oracle.c", "direct_oracle.c",
                                          "indirect_oracle.c", "mis_oracle.c", "power_oracle.c", "roulette_oracle.c", "ris_oracle.c",
                                          "env_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]

FEATURES = ("albedo", "normal", "depth", "emission")
# albedo, normal, depth, emission: float32 [frames, local pixels, 3]; tri, id, flipped: int32 [frames, local pixels] -- the triangle hit
# (-1: a miss), its id as stored, 1 when the normal was negated at :243
Samples = collections.namedtuple("Samples", "albedo normal depth emission tri id flipped")


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
        L.ofe_samples.restype, L.ofe_samples.argtypes = I, [V, I, V, I, V, F, F] + [I] * 7 + [V] * 5
        _lib = L
    return _lib


def local_pixels(W, H, stripe_rows=1, n_ranks=1, rank=0):
    """in closed form: H reaches 2^25 - 1 (tests/extent_cases.py), where a walk over the rows takes seconds"""
    return W * direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)


def samples(tris, mats, W, H, frames, *, frame_begin=0, cam=None, stripe_rows=1, n_ranks=1, rank=0) -> Samples:
    """the four sample arrays of frames [frame_begin, frame_begin + frames) and what lies behind them; cam: a Camera with its lens
    (None = the reference's)"""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    npix = local_pixels(W, H, stripe_rows, n_ranks, rank)
    out = [np.zeros((frames, npix, 3), np.float32) for _ in FEATURES]
    info = np.zeros((frames, npix, 3), np.int32)
    R, Fd = (0.0, 0.0) if cam is None else (cam.lens_radius, cam.focus_distance)
    rc = lib().ofe_samples(ptr(tris) if len(tris) else None, len(tris), ptr(mats), len(mats), ptr(cam10(cam)), R, Fd, W, H,
                           stripe_rows, n_ranks, rank, frame_begin, frames, *[ptr(a) for a in out], ptr(info))
    if rc != 0:
        raise ValueError("ofe_samples rejected the camera")
    return Samples(*out, info[..., 0].copy(), info[..., 1].copy(), info[..., 2].copy())


_ONCE = {}


def once(key, make) -> Samples:
    """``make()`` -- a case's Samples -- computed once per key, shared by every test that asks, read-only"""
    if key not in _ONCE:
        _ONCE[key] = make()
        for a in _ONCE[key]:
            a.setflags(write=False)
    return _ONCE[key]


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
