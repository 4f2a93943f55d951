"""Builds, loads and binds tests/libtest_roulette_oracle.so: the CPU oracle's Russian roulette (tests/roulette_oracle.c) -- the
framebuffer of pt_render_indirect_rr for each of its four estimators and, per sample, the radiance before the fold, the vertices reached,
why the path ended (ROULETTE beside indirect_oracle's reasons) and per vertex what the roulette did with its s, q and r.  A library of
its own (tests/roulette_oracles.c: the restatements it builds on, then roulette_oracle.c), so that tests/oracles.py, tests/power_oracle.py
and their libraries stay as they are.  TEST INFRASTRUCTURE.

``__graft_entry__.build()`` builds it (``python -B tests/roulette_oracle.py build``); ``lib()`` builds it again when it is missing or
older than one of its sources.
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
LIB_PATH = os.path.join(_HERE, "libtest_roulette_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("roulette_oracles.c", "roulette_oracle.c", "power_oracle.c", "camera_oracle.c", "direct_oracle.c",
                                          "indirect_oracle.c", "mis_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]

END_MISS, END_PDF, END_DEPTH, END_ROULETTE = 0, 1, 2, 3      # why a path ended (indirect_oracle's OII_END_*, ORR_END_ROULETTE)
RR_NONE, RR_PASS, RR_SURVIVED, RR_ENDED = 0, 1, 2, 3         # what the roulette did at a vertex (ORR_RR_*)
DETAIL_VERTICES = 16                                         # the vertex window of the per-vertex account
NEVER = 65535                                                # a first_bounce no path reaches (B <= 65535)

_SIGNATURES = {
    "orr_render": (I, [I, V, I, V, V, I, V, V, V, V] + [I] * 10 + [F, V]),
    "orr_samples": (I, [I, V, I, V, V, I, V, V, V, V, I, I, V, V, I64, I, I, I, F] + [V] * 7),
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


def _inputs(tris, mats, lights, power, counts, tab):
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    cn = light_counts(li, len(tris)) if counts is None else np.ascontiguousarray(counts, np.int32)
    if not power:
        cdf = tri_q = None
    elif tab is None:
        cdf, tri_q = power_oracle.table(tris, mats, li)
    else:
        cdf, tri_q = np.ascontiguousarray(tab[0], np.uint64), np.ascontiguousarray(tab[1], np.uint32)
    return tris, mats, li, cn, cdf, tri_q


def render(tris, mats, W, H, frame_begin, frame_count, K, B, R, cap, *, mis=False, power=False, lights=None, counts=None, tab=None, cam=None,
           stripe_rows=1, n_ranks=1, rank=0, start=None):
    """float32 [local pixels, 4]: the framebuffer of pt_render_indirect_rr with first_bounce ``R`` and max_survival ``cap`` for the
    estimator (``mis``, ``power``), in ``mis_oracle.render``'s layout.  counts / tab: None = made of the list."""
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, power, counts, tab)
    rows = direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)
    fb = np.zeros((rows * W, 4), np.float32) if start is None else np.array(start, np.float32).reshape(rows * W, 4).copy()
    c = cam10(cam)
    rc = lib().orr_render(int(bool(mis)), _p(tris), len(tris), ptr(mats), _p(li), len(li), _p(cdf), _p(tri_q), _p(cn), ptr(c), W, H, stripe_rows,
                          n_ranks, rank, frame_begin, frame_count, K, B, R, cap, ptr(fb))
    return None if rc != 0 else fb


def samples(tris, mats, W, H, gid, frame, K, B, R, cap, *, mis=False, power=False, lights=None, counts=None, tab=None, cam=None,
            details=False):
    """Per sample (gid[i], frame[i]): (radiance float32 [n, 3] before the fold, vertices int32 [n], end int32 [n, 2] = (END_*, the loop index
    at which the path ended)); with ``details`` also, for the first V = min(B, DETAIL_VERTICES) vertices, code uint8 [n, V] (RR_*) and the
    roulette's s, q, r, float32 [n, V] each (0 where it was not played)."""
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, power, counts, tab)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n, Vn = len(gid), min(B, DETAIL_VERTICES)
    rad = np.zeros((n, 3), np.float32)
    vertices = np.zeros(n, np.int32)
    end = np.zeros((n, 2), np.int32)
    code = np.zeros((n, Vn), np.uint8)
    s, q, r = (np.zeros((n, Vn), np.float32) for _ in range(3))
    c = cam10(cam)
    d = (ptr(code), ptr(s), ptr(q), ptr(r)) if details else (None,) * 4
    rc = lib().orr_samples(int(bool(mis)), _p(tris), len(tris), ptr(mats), _p(li), len(li), _p(cdf), _p(tri_q), _p(cn), ptr(c), W, H, ptr(gid),
                           ptr(frame), n, K, B, R, cap, ptr(rad), ptr(vertices), ptr(end), *d)
    if rc != 0:
        raise ValueError("orr_samples rejected the camera")
    return (rad, vertices, end, code, s, q, r) if details else (rad, vertices, end)


THREADS = max(1, min(16, os.cpu_count() or 1))


def sample_frames(tris, mats, W, H, frames, K, B, R, cap, *, mis=False, power=False, lights=None, frame_begin=0):
    """(radiance float64 [frames, W * H, 3], vertices int32 [frames, W * H], end int32 [frames, W * H]) of every sample of frames
    [frame_begin, frame_begin + frames), computed in slices on threads (the library holds no state) -- the result is that of one call."""
    lib()
    tris, mats, li, cn, cdf, tri_q = _inputs(tris, mats, lights, power, None, None)

    def run(span):
        gid, frame = all_samples(W, H, span[1] - span[0], span[0])
        return samples(tris, mats, W, H, gid, frame, K, B, R, cap, mis=mis, power=power, lights=li, counts=cn,
                       tab=None if cdf is None else (cdf, tri_q))

    step = max(1, -(-frames // (4 * THREADS)))
    spans = [(f, min(f + step, frame_begin + frames)) for f in range(frame_begin, frame_begin + frames, step)]
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(run, spans))
    rad = np.concatenate([p[0] for p in parts]).astype(np.float64).reshape(frames, W * H, 3)
    return rad, np.concatenate([p[1] for p in parts]).reshape(frames, W * H), np.concatenate([p[2][:, 0] for p in parts]).reshape(frames, W * H)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
