"""ctypes binding of tests/indirect_oracle.c: the CPU oracle's path tracing with light sampling at every vertex -- the framebuffer of
pt_render_indirect, and per sample the radiance before the fold, the vertices the path reached and why it ended (``samples``), or
what happened at each of its first vertices (``details``).  TEST INFRASTRUCTURE (the library: tests/oracles.py).
"""
from __future__ import annotations

import numpy as np

import direct_oracle
from oracles import I, I64, V, cam10, declare, lib, ptr

END_MISS, END_PDF, END_DEPTH = 0, 1, 2   # why a path ended (indirect_oracle.c: OII_END_*)

declare({
    "oii_render": (I, [V, I, V, V, I, V] + [I] * 9 + [V]),
    "oii_samples": (I, [V, I, V, V, I, V, I, I, V, V, I64, I, I, V, V, V, V]),
    "oii_details": (I, [V, I, V, V, I, V, I, I, V, V, I64, I, I, V, V, V, V, V, V, V, V]),
})


def render(tris, mats, W, H, frame_begin, frame_count, K, B, *, lights=None, cam=None, stripe_rows=1, n_ranks=1, rank=0, start=None):
    """float32 [local pixels, 4]: frames [frame_begin, frame_begin + frame_count) at ``B`` bounces and ``K`` light samples per
    vertex folded into ``start`` (or zeros); None when the camera is rejected.  lights: the light list (None = scene.emitters);
    cam: a Camera (None = the reference's)."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    rows = direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)
    fb = np.zeros((rows * W, 4), np.float32) if start is None else np.array(start, np.float32).reshape(rows * W, 4).copy()
    c = cam10(cam)
    rc = lib().oii_render(ptr(tris) if len(tris) else None, len(tris), ptr(mats), ptr(li) if len(li) else None, len(li), ptr(c),
                          W, H, stripe_rows, n_ranks, rank, frame_begin, frame_count, K, B, ptr(fb))
    return None if rc != 0 else fb


def samples(tris, mats, W, H, gid, frame, K, B, *, lights=None, cam=None):
    """Per sample (gid[i], frame[i]): the radiance before the fold (float32 [n, 3]), the vertices the path reached (int32 [n]), why
    it ended (uint8 [n]: END_MISS, END_PDF, END_DEPTH) and the light samples at vertices >= 2 whose shadow ray was open / occluded
    (int32 [n, 2])."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n = len(gid)
    rad = np.zeros((n, 3), np.float32)
    vertices = np.zeros(n, np.int32)
    end = np.zeros(n, np.uint8)
    later = np.zeros((n, 2), np.int32)
    c = cam10(cam)
    rc = lib().oii_samples(ptr(tris) if len(tris) else None, len(tris), ptr(mats), ptr(li) if len(li) else None, len(li), ptr(c),
                           W, H, ptr(gid), ptr(frame), n, K, B, ptr(rad), ptr(vertices), ptr(end), ptr(later))
    if rc != 0:
        raise ValueError("oii_samples rejected the camera")
    return rad, vertices, end, later


DETAIL_VERTICES = 8   # details() reports the first min(B, 8) vertices of a path


def details(tris, mats, W, H, gid, frame, K, B, *, lights=None, cam=None):
    """Per sample (gid[i], frame[i]), for the first V = min(B, 8) vertices of its path: the hit's material type (uint8 [n, V], 0 =
    the path has no such vertex), whether the normal was negated at :243 and whether the hit triangle's material is emissive (uint8
    [n, V] each), and the reason code of each light sample (uint8 [n, V, K]: direct_oracle's NOT_DRAWN .. R_OCCLUDED); then why the
    path ended and the loop index it happened at (int32 [n, 2]: END_*, i -- the search that missed, the vertex whose pdf <= 0, or
    B - 1), the radiance before the fold (float32 [n, 3]), whether a component of it is NaN or infinite (uint8 [n]), and last the
    hit's material index per vertex (int32 [n, V], -1 = no such vertex)."""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n, V = len(gid), min(B, DETAIL_VERTICES)
    mtype, flipped, emissive = (np.zeros((n, V), np.uint8) for _ in range(3))
    material = np.zeros((n, V), np.int32)
    reason = np.zeros((n, V, K), np.uint8)
    end = np.zeros((n, 2), np.int32)
    rad = np.zeros((n, 3), np.float32)
    nonfinite = np.zeros(n, np.uint8)
    c = cam10(cam)
    rc = lib().oii_details(ptr(tris) if len(tris) else None, len(tris), ptr(mats), ptr(li) if len(li) else None, len(li), ptr(c),
                           W, H, ptr(gid), ptr(frame), n, K, B, ptr(mtype), ptr(material), ptr(flipped), ptr(emissive), ptr(reason), ptr(end),
                           ptr(rad), ptr(nonfinite))
    if rc != 0:
        raise ValueError("oii_details rejected the camera")
    return mtype, flipped, emissive, reason, end, rad, nonfinite, material


def all_samples(W, H, frames, frame_begin=0):
    """(gid, frame) of every sample of ``frames`` frames, frame-major -- the order of the device's sample workspace"""
    gid = np.tile(np.arange(W * H, dtype=np.int32), frames)
    frame = np.repeat(np.arange(frame_begin, frame_begin + frames, dtype=np.int32), W * H)
    return gid, frame
