"""Builds, loads and binds tests/libtest_direct_oracle.so: the CPU oracle's direct illumination (tests/direct_oracle.c through the
translation unit tests/direct_oracles.c, which includes tests/oracles.c whole) -- the framebuffer of pt_render_direct, and the
per-light-sample decisions behind it with their reasons.  TEST INFRASTRUCTURE.

``__graft_entry__.build()`` builds it (``python -B tests/direct_oracle.py build``); ``lib()`` builds it again when it is missing or
older than one of its sources, as ``oracles.lib()`` does.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

import oracles
from oracles import cam10, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtest_direct_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("direct_oracles.c", "direct_oracle.c")] + list(oracles._SRCS)

NONE, OCCLUDED, OPEN = 0, 1, 2   # the decisions of a light sample (direct_oracle.c: ODI_*)
# why (direct_oracle.c: ODI_R_*): NONE is NOT_DRAWN (the primary ray missed, or no lights), NOT_FACING (cs <= 0), EDGE_ON (cl <= 0),
# NAN (cs or cl NaN) or OTHER_TYPE (:220); OPEN is OPEN_UNSEARCHED (tl <= 0) or R_OPEN; OCCLUDED is R_OCCLUDED
NOT_DRAWN, NOT_FACING, EDGE_ON, NAN, OTHER_TYPE, OPEN_UNSEARCHED, R_OPEN, R_OCCLUDED = range(8)
REASONS = ("NOT_DRAWN", "NOT_FACING", "EDGE_ON", "NAN", "OTHER_TYPE", "OPEN_UNSEARCHED", "OPEN", "OCCLUDED")
DECISION_OF = np.array([NONE, NONE, NONE, NONE, NONE, OPEN, OPEN, OCCLUDED], np.uint8)   # reason code -> decision

_V, _I, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_SIGNATURES = {
    "odi_render": (_I, [_V, _I, _V, _V, _I, _V] + [_I] * 8 + [_V]),
    "odi_decisions": (_I, [_V, _I, _V, _V, _I, _V, _I, _I, _V, _V, _I64, _I, _V, _V, _V]),
    "odi_details": (_I, [_V, _I, _V, _V, _I, _V, _I, _I, _V, _V, _I64, _I, _V, _V, _V, _V, _V]),
}


def build() -> str:
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc] + oracles.CFLAGS + ["-shared", "-o", LIB_PATH, _SRCS[0], "-lm", "-lpthread"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(f) for f in _SRCS):
            build()
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _lights(tris, mats, lights):
    if lights is None:
        from oclpathtracer_amd import scene

        lights = scene.emitters(tris, mats)
    return np.ascontiguousarray(lights, np.int32)


def render(tris, mats, W, H, frame_begin, frame_count, K, *, lights=None, cam=None, stripe_rows=1, n_ranks=1, rank=0, start=None):
    """float32 [local pixels, 4]: frames [frame_begin, frame_begin + frame_count) folded into ``start`` (or zeros); None when the
    camera is rejected.  lights: the light list (None = scene.emitters); cam: a Camera (None = the reference's)."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = _lights(tris, mats, lights)
    rows = sum(1 for r in range(H) if (r // stripe_rows) % n_ranks == rank)
    fb = np.zeros((rows * W, 4), np.float32) if start is None else np.array(start, np.float32).reshape(rows * W, 4).copy()
    c = cam10(cam)
    rc = lib().odi_render(ptr(tris) if len(tris) else None, len(tris), ptr(mats), ptr(li) if len(li) else None, len(li), ptr(c),
                          W, H, stripe_rows, n_ranks, rank, frame_begin, frame_count, K, ptr(fb))
    return None if rc != 0 else fb


def decisions(tris, mats, W, H, gid, frame, K, *, lights=None, cam=None):
    """Per sample (gid[i], frame[i]): hit (uint8 [n]), the decision of each light sample (uint8 [n, K]: NONE, OCCLUDED, OPEN) and
    the sample's radiance L (float32 [n, 3])."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = _lights(tris, mats, lights)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    hit = np.zeros(len(gid), np.uint8)
    dec = np.zeros((len(gid), K), np.uint8)
    rad = np.zeros((len(gid), 3), np.float32)
    c = cam10(cam)
    rc = lib().odi_decisions(ptr(tris) if len(tris) else None, len(tris), ptr(mats), ptr(li) if len(li) else None, len(li), ptr(c),
                             W, H, ptr(gid), ptr(frame), len(gid), K, ptr(hit), ptr(dec), ptr(rad))
    if rc != 0:
        raise ValueError("odi_decisions rejected the camera")
    return hit, dec, rad


def details(tris, mats, W, H, gid, frame, K, *, lights=None, cam=None):
    """Per sample (gid[i], frame[i]): hit and flipped (uint8 [n]: the normal was negated at :243), the reason code of each light
    sample (uint8 [n, K], see REASONS; DECISION_OF[reason] is what ``decisions`` returns) with its d2 (float32 [n, K], -1 where
    no sample was drawn) and the sample's radiance L (float32 [n, 3])."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = _lights(tris, mats, lights)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n = len(gid)
    hit, flipped = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    reason = np.zeros((n, K), np.uint8)
    d2 = np.zeros((n, K), np.float32)
    rad = np.zeros((n, 3), np.float32)
    c = cam10(cam)
    rc = lib().odi_details(ptr(tris) if len(tris) else None, len(tris), ptr(mats), ptr(li) if len(li) else None, len(li), ptr(c),
                           W, H, ptr(gid), ptr(frame), n, K, ptr(hit), ptr(flipped), ptr(reason), ptr(d2), ptr(rad))
    if rc != 0:
        raise ValueError("odi_details rejected the camera")
    return hit, flipped, reason, d2, rad


def local_gids(W, H, stripe_rows=1, n_ranks=1, rank=0):
    """the global pixel index of every local pixel of ``rank`` in the stripe layout, in the framebuffer's order"""
    rows = [r for r in range(H) if (r // stripe_rows) % n_ranks == rank]
    return (np.asarray(rows, np.int64)[:, None] * W + np.arange(W)[None, :]).reshape(-1)


def count_reasons(reason):
    """{name: how many light samples ended for that reason}"""
    return {name: int((reason == k).sum()) for k, name in enumerate(REASONS)}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
