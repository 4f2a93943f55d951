"""ctypes binding of tests/query_oracle.c: the CPU oracle's closest hit (with u, v, material and the caller's tmax) and camera
rays, in the record layouts of pt_intersect_rays / pt_camera_rays.  TEST INFRASTRUCTURE.

Compiled on demand with oracle/Makefile's flags, as tests/camera_oracle.py does.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libquery_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("query_oracle.c", "camera_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]


def build() -> str:
    from camera_oracle import CFLAGS

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
        L.oq_closest.restype = None
        L.oq_closest.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        L.oq_camera_rays.restype = ctypes.c_int
        L.oq_camera_rays.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.oq_all_hits.restype = ctypes.c_int64
        L.oq_all_hits.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 3
        L.oq_get_rays.restype = None
        L.oq_get_rays.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        _lib = L
    return _lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def closest(tris: np.ndarray, rays: np.ndarray) -> np.ndarray:
    """rays: float32 [N, 8] (pt_ray words) -> float32 [N, 12] (pt_hit words; tri and material as int32 bits)."""
    tris = np.ascontiguousarray(tris)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    out = np.zeros((len(rays), 12), np.float32)
    lib().oq_closest(_ptr(tris) if len(tris) else None, len(tris), _ptr(rays), len(rays), _ptr(out))
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
        m = lib().oq_all_hits(_ptr(tris) if len(tris) else None, len(tris), _ptr(rays), len(rays), cap, _ptr(ray), _ptr(tri), _ptr(t))
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
    lib().oq_get_rays(_ptr(rays), len(rays), _ptr(out))
    return out


def camera_rays(W: int, H: int, frame: int, cam=None):
    """float32 [W * H, 8] pt_ray words, or None when the camera is rejected; cam: a Camera (None = the reference's)."""
    out = np.zeros((W * H, 8), np.float32)
    c = None
    if cam is not None:
        c = np.array(list(cam.eye) + list(cam.center) + list(cam.up) + [cam.fov_y_deg], np.float32)
    rc = lib().oq_camera_rays(_ptr(c) if c is not None else None, W, H, frame, _ptr(out))
    return None if rc != 0 else out
