"""ctypes binding of tests/primary_accept.c: per pixel the triangles the reference's test ACCEPTS for a sample's primary ray, and those
that only pass the cull and the u test.  TEST INFRASTRUCTURE (the library: tests/oracles.py).
"""
from __future__ import annotations

import numpy as np

from oracles import I, I64, V, cam10, declare, lib, ptr

declare({
    "opa_union": (I, [V, I, V, I, I, I, I, V, I64, V, V, V]),
})


def union(tris, W, H, frames, *, cam=None, gid=None, frame_begin=0):
    """Over frames [frame_begin, frame_begin + frames) of every pixel in ``gid`` (global pixel indices; None = the whole image):
    (accepted, reach_u, n_accepted, n_reach_u) -- two uint64 arrays, bit j = triangle j, the per-pixel UNIONS of the triangles the
    reference accepts / lets past the u test, and the numbers of such (sample, triangle) pairs summed over all those samples.
    cam: a Camera (None = the reference's built-in one)."""
    tris = np.ascontiguousarray(tris)
    gid = np.arange(W * H, dtype=np.int32) if gid is None else np.ascontiguousarray(gid, np.int32)
    acc = np.zeros(len(gid), np.uint64)
    ru = np.zeros(len(gid), np.uint64)
    counts = np.zeros(2, np.uint64)
    c = cam10(cam)
    rc = lib().opa_union(ptr(tris) if len(tris) else None, len(tris), ptr(c), W, H, frame_begin, frames, ptr(gid), len(gid),
                         ptr(acc), ptr(ru), ptr(counts))
    if rc != 0:
        raise ValueError("opa_union rejected the camera or the triangle count")
    return acc, ru, int(counts[0]), int(counts[1])


def popcount(a) -> np.ndarray:
    """set bits of each uint64"""
    return np.unpackbits(np.ascontiguousarray(a, np.uint64).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def mask_bits(snapshot, ntri) -> np.ndarray:
    """The device's mask table (uint32 [pixels, 2]: word c holds triangles [32 c, 32 c + n), n = min(32, ntri - 32 c), triangle
    32 c + j at bit n - 1 - j) as uint64 sets with triangle j at bit j, the restatement's order."""
    snap = np.asarray(snapshot, np.uint32).reshape(-1, 2)
    out = np.zeros(len(snap), np.uint64)
    for j in range(ntri):
        c = j >> 5
        n = min(32, ntri - 32 * c)
        bit = (snap[:, c] >> np.uint32(n - 1 - (j & 31))) & np.uint32(1)
        out |= bit.astype(np.uint64) << np.uint64(j)
    return out
