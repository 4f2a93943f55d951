"""ctypes binding of tests/mis_oracle.c: the CPU oracle's path tracing with light sampling at every vertex and multiple importance
sampling -- the framebuffer of pt_render_indirect_mis, and per sample the radiance before the fold with what
``indirect_oracle.samples`` says and the sample's weighted light samples and later emissive hits (``samples``), or what happened at
each of its first vertices (``details``).  ``counts`` is an input of every entry point, as it is of the device's: None makes it of
the list as pt_light_counts does (``light_counts``).  TEST INFRASTRUCTURE (the library: tests/oracles.py).
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import direct_oracle
import indirect_oracle
from indirect_oracle import DETAIL_VERTICES, all_samples   # noqa: F401  (the same sample order and vertex window)
from oracles import I, I64, V, cam10, declare, lib, ptr

W_NONE, WEIGHTED, LAST_VERTEX, BACK_SIDE = 0, 1, 2, 3   # what became of a light sample's weight (mis_oracle.c: OMI_W_*)

declare({
    "omi_render": (I, [V, I, V, V, I, V, V] + [I] * 9 + [V]),
    "omi_samples": (I, [V, I, V, V, I, V, V, I, I, V, V, I64, I, I] + [V] * 5),
    "omi_details": (I, [V, I, V, V, I, V, V, I, I, V, V, I64, I, I] + [V] * 11),
})


def light_counts(lights, num_triangles) -> np.ndarray:
    """int32 [num_triangles]: how many entries of ``lights``, each clamped into [0, num_triangles), name each triangle -- what
    pt_light_counts writes"""
    li = np.asarray(lights, np.int64)
    if num_triangles == 0:
        return np.zeros(0, np.int32)
    return np.bincount(np.clip(li, 0, num_triangles - 1), minlength=num_triangles).astype(np.int32)


def _inputs(tris, mats, lights, counts):
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    cn = light_counts(li, len(tris)) if counts is None else np.ascontiguousarray(counts, np.int32)
    assert len(cn) >= len(tris) or len(li) == 0, "counts holds one entry per triangle"
    return tris, mats, li, cn


def _p(a):
    return ptr(a) if len(a) else None


def render(tris, mats, W, H, frame_begin, frame_count, K, B, *, lights=None, counts=None, cam=None, stripe_rows=1, n_ranks=1, rank=0,
           start=None):
    """float32 [local pixels, 4]: ``indirect_oracle.render`` for the MIS estimator.  counts: int32 [num_triangles] (None = made of
    the list)."""
    tris, mats, li, cn = _inputs(tris, mats, lights, counts)
    rows = direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)
    fb = np.zeros((rows * W, 4), np.float32) if start is None else np.array(start, np.float32).reshape(rows * W, 4).copy()
    c = cam10(cam)
    rc = lib().omi_render(_p(tris), len(tris), ptr(mats), _p(li), len(li), _p(cn), ptr(c), W, H, stripe_rows, n_ranks, rank,
                          frame_begin, frame_count, K, B, ptr(fb))
    return None if rc != 0 else fb


def samples(tris, mats, W, H, gid, frame, K, B, *, lights=None, counts=None, cam=None):
    """``indirect_oracle.samples``' four arrays for the MIS estimator, then int32 [n, 2]: the light samples of the whole path whose
    weight took the MIS factor, and the path's vertices i >= 1 on an emissive material."""
    tris, mats, li, cn = _inputs(tris, mats, lights, counts)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n = len(gid)
    rad = np.zeros((n, 3), np.float32)
    vertices = np.zeros(n, np.int32)
    end = np.zeros(n, np.uint8)
    later = np.zeros((n, 2), np.int32)
    mis = np.zeros((n, 2), np.int32)
    c = cam10(cam)
    rc = lib().omi_samples(_p(tris), len(tris), ptr(mats), _p(li), len(li), _p(cn), ptr(c), W, H, ptr(gid), ptr(frame), n, K, B,
                           ptr(rad), ptr(vertices), ptr(end), ptr(later), ptr(mis))
    if rc != 0:
        raise ValueError("omi_samples rejected the camera")
    return rad, vertices, end, later, mis


def details(tris, mats, W, H, gid, frame, K, B, *, lights=None, counts=None, cam=None):
    """``indirect_oracle.details``' eight arrays for the MIS estimator (mtype, flipped, emissive, reason, end, radiance, nonfinite,
    material), then per light sample what became of its weight (uint8 [n, V, K]: W_NONE where it did not reach its weight, WEIGHTED,
    LAST_VERTEX, BACK_SIDE), and per vertex counts[h] of a later emissive hit (int32 [n, V], -1 = none) and its weight wb (float32
    [n, V])."""
    tris, mats, li, cn = _inputs(tris, mats, lights, counts)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n, V = len(gid), min(B, DETAIL_VERTICES)
    mtype, flipped, emissive = (np.zeros((n, V), np.uint8) for _ in range(3))
    material = np.zeros((n, V), np.int32)
    reason = np.zeros((n, V, K), np.uint8)
    weight = np.zeros((n, V, K), np.uint8)
    end = np.zeros((n, 2), np.int32)
    rad = np.zeros((n, 3), np.float32)
    nonfinite = np.zeros(n, np.uint8)
    count = np.zeros((n, V), np.int32)
    wb = np.zeros((n, V), np.float32)
    c = cam10(cam)
    rc = lib().omi_details(_p(tris), len(tris), ptr(mats), _p(li), len(li), _p(cn), ptr(c), W, H, ptr(gid), ptr(frame), n, K, B,
                           ptr(mtype), ptr(material), ptr(flipped), ptr(emissive), ptr(reason), ptr(end), ptr(rad), ptr(nonfinite),
                           ptr(weight), ptr(count), ptr(wb))
    if rc != 0:
        raise ValueError("omi_details rejected the camera")
    return mtype, flipped, emissive, reason, end, rad, nonfinite, material, weight, count, wb


THREADS = max(1, min(16, os.cpu_count() or 1))


def radiance_frames(tris, mats, W, H, frame_begin, frames, K, B, *, lights=None, counts=None, mis=True):
    """float64 [frames, W * H, 3]: the radiance before the fold of every sample of frames [frame_begin, frame_begin + frames), of
    this restatement or (``mis=False``) of ``indirect_oracle``.  A sample depends on nothing but its pixel and frame, so the frames
    are computed in slices on threads (the library holds no state; ctypes releases the interpreter) -- the result is that of one
    call."""
    lib()   # loaded before the threads start

    def run(span):
        gid, frame = all_samples(W, H, span[1] - span[0], span[0])
        if mis:
            return samples(tris, mats, W, H, gid, frame, K, B, lights=lights, counts=counts)[0]
        return indirect_oracle.samples(tris, mats, W, H, gid, frame, K, B, lights=lights)[0]

    step = max(1, -(-frames // (4 * THREADS)))
    spans = [(f, min(f + step, frame_begin + frames)) for f in range(frame_begin, frame_begin + frames, step)]
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(run, spans))
    return np.concatenate(parts).astype(np.float64).reshape(frames, W * H, 3)
