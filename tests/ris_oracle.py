"""Builds, loads and binds tests/libtest_ris_oracle.so: the CPU oracle's resampled light sampling (tests/ris_oracle.c) -- the framebuffer
of pt_render_direct_ris and pt_render_indirect_ris and, per sample, the radiance before the fold and per light sample which candidate
was kept, wsum, s_sel, how many candidates had s > 0, how often a later one replaced a kept one, the reason code of the kept one's ray
and its MIS weight code.  A library of its own (tests/ris_oracles.c: the restatements it builds on, then ris_oracle.c), so that
tests/oracles.py, tests/power_oracle.py, tests/roulette_oracle.py and their libraries stay as they are.  TEST INFRASTRUCTURE.

``__graft_entry__.build()`` builds it (``python -B tests/ris_oracle.py build``); ``lib()`` builds it again when it is missing or older
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
import power_oracle
from indirect_oracle import all_samples
from mis_oracle import light_counts
from oracles import CFLAGS, F, I, I64, V, cam10, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtest_ris_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("ris_oracles.c", "ris_oracle.c", "roulette_oracle.c", "power_oracle.c", "camera_oracle.c",
                                          "direct_oracle.c", "indirect_oracle.c", "mis_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]

# a light sample's reason: the kept candidate's ray (direct_oracle's ODI_R_*), NONE when no candidate was kept
R_NOT_DRAWN, R_OPEN_UNSEARCHED, R_OPEN, R_OCCLUDED, R_NONE = 0, 5, 6, 7, 9
W_NONE, W_WEIGHTED, W_LAST_VERTEX, W_BACK_SIDE = 0, 1, 2, 3   # mis_oracle's OMI_W_* of the kept candidate
DETAIL_VERTICES = 8
NEVER = 65535                                                  # a first_bounce no path reaches: no roulette
MAX_CANDIDATES = 32

_SIGNATURES = {
    "ors_render": (I, [I, I, V, I, V, V, I, V, V, V, V] + [I] * 10 + [F, I, V]),
    "ors_samples": (I, [I, I, V, I, V, V, I, V, V, V, V, I, I, V, V, I64, I, I, I, F, I] + [V] * 8),
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
    return ptr(a) if a is not None and len(a) else None


def _inputs(tris, mats, lights, counts, tab):
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    cn = light_counts(li, len(tris)) if counts is None else np.ascontiguousarray(counts, np.int32)
    if tab is None:
        cdf, tri_q = power_oracle.table(tris, mats, li)
    else:
        cdf, tri_q = np.ascontiguousarray(tab[0], np.uint64), np.ascontiguousarray(tab[1], np.uint32)
    return tris, mats, li, cn, cdf, tri_q


def render(tris, mats, W, H, frame_begin, frame_count, K, M, *, B=None, R=NEVER, cap=1.0, mis=False, lights=None, counts=None, tab=None,
           cam=None, stripe_rows=1, n_ranks=1, rank=0, start=None):
    """float32 [local pixels, 4]: the framebuffer of pt_render_direct_ris (``B`` None) or of pt_render_indirect_ris with max_bounces ``B``,
    the roulette (``R``, ``cap``) and ``mis``, with ``M`` candidates, in ``roulette_oracle.render``'s layout.  counts / tab: None = made of
    the list."""
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, counts, tab)
    rows = direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)
    fb = np.zeros((rows * W, 4), np.float32) if start is None else np.array(start, np.float32).reshape(rows * W, 4).copy()
    c = cam10(cam)
    rc = lib().ors_render(int(B is not None), int(bool(mis)), _p(tris), len(tris), ptr(mats), _p(li), len(li), ptr(cdf), _p(tri_q), _p(cn), ptr(c),
                          W, H, stripe_rows, n_ranks, rank, frame_begin, frame_count, K, B or 1, R, cap, M, ptr(fb))
    if rc == -2:
        raise ValueError("ors_render: candidates outside 1..32")
    return None if rc != 0 else fb


DETAIL_NAMES = ("kept", "wsum", "ssel", "positive", "replaced", "reason", "wcode")


def samples(tris, mats, W, H, gid, frame, K, M, *, B=None, R=NEVER, cap=1.0, mis=False, lights=None, counts=None, tab=None, cam=None,
            details=False):
    """Per sample (gid[i], frame[i]): radiance float32 [n, 3] before the fold; with ``details`` (radiance, dict) where the dict holds, for
    the first V = 1 (direct) or min(B, DETAIL_VERTICES) vertices and each light sample, arrays [n, V, K]: kept (the kept candidate's index,
    -1: none), wsum, ssel, positive (candidates with s > 0), replaced (how often a later candidate replaced a kept one), reason (R_*) and
    wcode (W_* of the kept one)."""
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, counts, tab)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n, Vn = len(gid), 1 if B is None else min(B, DETAIL_VERTICES)
    rad = np.zeros((n, 3), np.float32)
    shape = (n, Vn, K)
    d = dict(kept=np.zeros(shape, np.int32), wsum=np.zeros(shape, np.float32), ssel=np.zeros(shape, np.float32),
             positive=np.zeros(shape, np.int32), replaced=np.zeros(shape, np.int32), reason=np.zeros(shape, np.uint8),
             wcode=np.zeros(shape, np.uint8))
    c = cam10(cam)
    dp = tuple(ptr(d[k]) for k in DETAIL_NAMES) if details else (None,) * 7
    rc = lib().ors_samples(int(B is not None), int(bool(mis)), _p(tris), len(tris), ptr(mats), _p(li), len(li), ptr(cdf), _p(tri_q), _p(cn),
                           ptr(c), W, H, ptr(gid), ptr(frame), n, K, B or 1, R, cap, M, ptr(rad), *dp)
    if rc != 0:
        raise ValueError("ors_samples rejected the camera or the candidates")
    return (rad, d) if details else rad


THREADS = max(1, min(16, os.cpu_count() or 1))


def sample_frames(tris, mats, W, H, frames, K, M, *, B=None, R=NEVER, cap=1.0, mis=False, lights=None, frame_begin=0):
    """radiance float64 [frames, W * H, 3] of every sample of frames [frame_begin, frame_begin + frames), computed in slices on threads
    (the library holds no state) -- the result is that of one call."""
    lib()
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, None, None)

    def run(span):
        gid, frame = all_samples(W, H, span[1] - span[0], span[0])
        return samples(tris, mats, W, H, gid, frame, K, M, B=B, R=R, cap=cap, mis=mis, lights=li, counts=cn, tab=(cdf, tri_q))

    step = max(1, -(-frames // (4 * THREADS)))
    spans = [(f, min(f + step, frame_begin + frames)) for f in range(frame_begin, frame_begin + frames, step)]
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(run, spans))
    return np.concatenate(parts).astype(np.float64).reshape(frames, W * H, 3)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
