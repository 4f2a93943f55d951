"""ctypes binding of tests/query_oracle.c: the CPU oracle's closest hit (with u, v, material and the caller's tmax) and camera
rays, in the record layouts of pt_intersect_rays / pt_camera_rays.  TEST INFRASTRUCTURE (the library: tests/oracles.py).
"""
from __future__ import annotations

import numpy as np

from oracles import I, I64, V, cam10, declare, lib, ptr

declare({
    "oq_closest": (None, [V, I, V, I64, V]),
    "oq_camera_rays": (I, [V, I, I, I, V]),
    "oq_all_hits": (I64, [V, I, V, I64, I64, V, V, V]),
    "oq_get_rays": (None, [V, I64, V]),
})


def closest(tris: np.ndarray, rays: np.ndarray) -> np.ndarray:
    """rays: float32 [N, 8] (pt_ray words) -> float32 [N, 12] (pt_hit words; tri and material as int32 bits)."""
    tris = np.ascontiguousarray(tris)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    out = np.zeros((len(rays), 12), np.float32)
    lib().oq_closest(ptr(tris) if len(tris) else None, len(tris), ptr(rays), len(rays), ptr(out))
    return out


def _blocks(n: int, threads: int):
    return [b for b in np.array_split(np.arange(n), max(1, min(threads, n // 4096 + 1))) if len(b)]


def closest_threads(tris: np.ndarray, rays: np.ndarray, threads: int = 8) -> np.ndarray:
    """closest() over blocks of rays on several host threads (the library call holds no Python lock): the same records."""
    from concurrent.futures import ThreadPoolExecutor

    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    lib()
    blocks = _blocks(len(rays), threads)
    if not blocks:
        return np.zeros((0, 12), np.float32)
    with ThreadPoolExecutor(len(blocks)) as ex:
        return np.concatenate(list(ex.map(lambda b: closest(tris, rays[b[0]: b[-1] + 1]), blocks)))


def _all_hits_block(tris, rays):
    cap = max(2 * len(rays), 1024)
    while True:
        ray, tri, t = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        m = lib().oq_all_hits(ptr(tris) if len(tris) else None, len(tris), ptr(rays), len(rays), cap, ptr(ray), ptr(tri), ptr(t))
        if m <= cap:
            return ray[:m], tri[:m], t[:m]
        cap = int(m)


def all_hits(tris: np.ndarray, rays: np.ndarray, threads: int = 8):
    """Every (ray, triangle, t) the exact test accepts at 0 < t < min(tmax, 1e20): int64 [M], int32 [M], float32 [M], rays
    ascending and triangles ascending within a ray."""
    from concurrent.futures import ThreadPoolExecutor

    tris = np.ascontiguousarray(tris)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    lib()
    blocks = _blocks(len(rays), threads)
    if not blocks:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    with ThreadPoolExecutor(len(blocks)) as ex:
        parts = list(ex.map(lambda b: _all_hits_block(tris, rays[b[0]: b[-1] + 1]), blocks))
    return (np.concatenate([p[0] + b[0] for p, b in zip(parts, blocks)]), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]))


def get_rays(rays: np.ndarray) -> np.ndarray:
    """float32 [N, 6]: each ray's origin and the normalised direction the oracle's getRay makes of it."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    out = np.zeros((len(rays), 6), np.float32)
    lib().oq_get_rays(ptr(rays), len(rays), ptr(out))
    return out


def camera_rays(W: int, H: int, frame: int, cam=None):
    """float32 [W * H, 8] pt_ray words, or None when the camera is rejected; cam: a Camera (None = the reference's)."""
    out = np.zeros((W * H, 8), np.float32)
    c = cam10(cam)
    rc = lib().oq_camera_rays(ptr(c), W, H, frame, ptr(out))
    return None if rc != 0 else out
