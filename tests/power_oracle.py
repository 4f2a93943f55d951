"""Builds, loads and binds tests/libtest_power_oracle.so: the CPU oracle's light choice by power (tests/power_oracle.c) -- the table
of pt_light_table, the framebuffers of pt_render_direct_power and pt_render_indirect_power, and per sample the radiance before the fold
with, per light sample, the entry chosen, its q and why it ended as it did.  A library of its own (tests/power_oracles.c: the
restatements it builds on, then power_oracle.c), so that tests/oracles.py and its library stay as they are.  TEST INFRASTRUCTURE.

``__graft_entry__.build()`` builds it (``python -B tests/power_oracle.py build``); ``lib()`` builds it again when it is missing or older
than one of its sources.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import direct_oracle
from indirect_oracle import DETAIL_VERTICES, all_samples   # noqa: F401  (the same sample order and vertex window)
from mis_oracle import light_counts
from oracles import CFLAGS, I, I64, V, cam10, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtest_power_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("power_oracles.c", "power_oracle.c", "camera_oracle.c", "direct_oracle.c", "indirect_oracle.c",
                                          "mis_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]

DIRECT, INDIRECT, MIS = 0, 1, 2   # the estimator (power_oracle.c: OPW_*)
EMPTY_TABLE = 8                   # a light sample's reason beside direct_oracle's: the table's total is 0 (OPW_R_EMPTY_TABLE)

_SIGNATURES = {
    "opw_table": (I, [V, I, V, I, V, I, V, V]),
    "opw_render": (I, [I, V, I, V, V, I, V, V, V, V] + [I] * 9 + [V]),
    "opw_samples": (I, [I, V, I, V, V, I, V, V, V, V, I, I, V, V, I64, I, I] + [V] * 5),
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
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _p(a):
    return ptr(a) if len(a) else None


def table(tris, mats, lights, num_triangles=None):
    """(cdf uint64 [nl + 1], tri_q uint32 [num_triangles]) of pt_light_table for ``lights`` (any int32 values: they are clamped) over the
    first ``num_triangles`` records of ``tris``."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = np.ascontiguousarray(lights, np.int32)
    ntri = len(tris) if num_triangles is None else int(num_triangles)
    cdf = np.zeros(len(li) + 1, np.uint64)
    tri_q = np.zeros(ntri, np.uint32)
    rc = lib().opw_table(_p(tris), ntri, ptr(mats), len(mats), _p(li), len(li), ptr(cdf), _p(tri_q))
    assert rc == 0
    return cdf, tri_q


def _inputs(tris, mats, lights, counts, tab):
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    cn = light_counts(li, len(tris)) if counts is None else np.ascontiguousarray(counts, np.int32)
    cdf, tri_q = table(tris, mats, li) if tab is None else (np.ascontiguousarray(tab[0], np.uint64), np.ascontiguousarray(tab[1], np.uint32))
    return tris, mats, li, cn, cdf, tri_q


def render(mode, tris, mats, W, H, frame_begin, frame_count, K, B=1, *, lights=None, counts=None, tab=None, cam=None, stripe_rows=1,
           n_ranks=1, rank=0, start=None):
    """float32 [local pixels, 4]: the framebuffer of pt_render_direct_power (``mode`` DIRECT) or pt_render_indirect_power (INDIRECT, MIS)
    in ``mis_oracle.render``'s layout.  counts / tab: None = made of the list."""
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, counts, tab)
    rows = direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)
    fb = np.zeros((rows * W, 4), np.float32) if start is None else np.array(start, np.float32).reshape(rows * W, 4).copy()
    c = cam10(cam)
    rc = lib().opw_render(mode, _p(tris), len(tris), ptr(mats), _p(li), len(li), ptr(cdf), _p(tri_q), _p(cn), ptr(c), W, H, stripe_rows,
                          n_ranks, rank, frame_begin, frame_count, K, B, ptr(fb))
    return None if rc != 0 else fb


def samples(mode, tris, mats, W, H, gid, frame, K, B=1, *, lights=None, counts=None, tab=None, cam=None, details=False):
    """Per sample (gid[i], frame[i]) the radiance before the fold, float32 [n, 3]; with ``details`` also, for the first V vertices (1 for
    DIRECT, min(B, 8) otherwise): entry int32 [n, V, K] (the list entry a light sample chose; -1 = not drawn or an empty table), q uint32
    [n, V, K], reason uint8 [n, V, K] (direct_oracle's codes and EMPTY_TABLE) and later int32 [n, V] (counts[h] of the MIS estimator's
    later emissive hit; -1 = none)."""
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, counts, tab)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n, Vn = len(gid), 1 if mode == DIRECT else min(B, DETAIL_VERTICES)
    rad = np.zeros((n, 3), np.float32)
    entry = np.zeros((n, Vn, K), np.int32)
    q = np.zeros((n, Vn, K), np.uint32)
    reason = np.zeros((n, Vn, K), np.uint8)
    later = np.zeros((n, Vn), np.int32)
    c = cam10(cam)
    d = (ptr(entry), ptr(q), ptr(reason), ptr(later)) if details else (None,) * 4
    rc = lib().opw_samples(mode, _p(tris), len(tris), ptr(mats), _p(li), len(li), ptr(cdf), _p(tri_q), _p(cn), ptr(c), W, H, ptr(gid),
                           ptr(frame), n, K, B, ptr(rad), *d)
    if rc != 0:
        raise ValueError("opw_samples rejected the camera")
    return (rad, entry, q, reason, later) if details else rad


THREADS = max(1, min(16, os.cpu_count() or 1))


def radiance_frames(mode, tris, mats, W, H, frames, K, B=1, *, lights=None):
    """float64 [frames, W * H, 3]: the radiance before the fold of every sample of frames [0, frames), computed in slices on threads (the
    library holds no state) -- the result is that of one call."""
    lib()
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, None, None)

    def run(span):
        gid, frame = all_samples(W, H, span[1] - span[0], span[0])
        return samples(mode, tris, mats, W, H, gid, frame, K, B, lights=li, counts=cn, tab=(cdf, tri_q))

    step = max(1, -(-frames // (4 * THREADS)))
    spans = [(f, min(f + step, frames)) for f in range(0, frames, step)]
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(run, spans))
    return np.concatenate(parts).astype(np.float64).reshape(frames, W * H, 3)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
