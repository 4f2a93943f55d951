"""Builds, loads and binds tests/libtest_env_oracle.so: the CPU oracle's environment lighting (tests/env_oracle.c) -- pt_env_table's table,
the two mappings of the octahedral map, the framebuffer of pt_render_direct_env and pt_render_indirect_env and, per sample, the radiance
before the fold and the account of its environment samples and misses.  A library of its own (tests/env_oracles.c: the restatements it
builds on, then env_oracle.c), so that the other oracle libraries stay as they are.  TEST INFRASTRUCTURE.

``__graft_entry__.build()`` builds it (``python -B tests/env_oracle.py build``); ``lib()`` builds it again when it is missing or older
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
LIB_PATH = os.path.join(_HERE, "libtest_env_oracle.so")
_SRCS = [os.path.join(_HERE, f) for f in ("env_oracles.c", "env_oracle.c", "roulette_oracle.c", "power_oracle.c", "camera_oracle.c",
                                          "direct_oracle.c", "indirect_oracle.c", "mis_oracle.c")] + \
        [os.path.join(os.path.dirname(_HERE), "oracle", f) for f in ("pt_oracle.c", "ptor_constants.h")]

# why an environment sample ended (OEV_R_*)
R_NOT_DRAWN, R_BELOW_HORIZON, R_OTHER_TYPE, R_EMPTY_TABLE, R_OPEN, R_OCCLUDED, R_NAN = range(7)
REASONS = ("NOT_DRAWN", "BELOW_HORIZON", "OTHER_TYPE", "EMPTY_TABLE", "OPEN", "OCCLUDED", "NAN")
DETAIL_VERTICES = 8
NEVER = 65535   # a first_bounce no path reaches: no roulette

_SIGNATURES = {
    "oev_texels": (I, [V, I64, I, V]),
    "oev_directions": (I, [V, I64, V, V]),
    "oev_table": (I, [V, I, V]),
    "oev_sample_at": (I, [V, V, I, I, I, I, I, V, F, V, V, V, ctypes.c_uint32, V, V]),
    "oev_render": (I, [I, V, I, V, V, I, V, V, V, V, V, I, I, V] + [I] * 9 + [I, F, V]),
    "oev_samples": (I, [I, V, I, V, V, I, V, V, V, V, V, I, I, V, I, I, V, V, I64, I, I, I, F] + [V] * 5),
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


def texels4(texels):
    """the map as the ABI takes it: float32 [N * N, 4] of an (N, N, 3 or 4) or [N * N, 3 or 4] array"""
    t = np.asarray(texels, np.float32)
    t = t.reshape(-1, t.shape[-1])
    out = np.zeros((len(t), 4), np.float32)
    out[:, :t.shape[1]] = t
    return out


def size_of(texels):
    n = int(round(np.sqrt(len(texels4(texels)))))
    assert n * n == len(texels4(texels)), "the map is not square"
    return n


def texel_of(dirs, N):
    """uint32 [n]: the texel of each direction float32 [n, 3] (any float)"""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out = np.zeros(len(d), np.uint32)
    assert lib().oev_texels(ptr(d), len(d), N, ptr(out)) == 0
    return out


def direction_of(ab):
    """(direction float32 [n, 3], r float32 [n]) of each point (a, b) float32 [n, 2] of the square"""
    p = np.ascontiguousarray(ab, np.float32).reshape(-1, 2)
    d, r = np.zeros((len(p), 3), np.float32), np.zeros(len(p), np.float32)
    assert lib().oev_directions(ptr(p), len(p), ptr(d), ptr(r)) == 0
    return d, r


def table(texels):
    """uint64 [N * N + 1]: pt_env_table's cdf"""
    t = texels4(texels)
    N = size_of(t)
    cdf = np.zeros(N * N + 1, np.uint64)
    assert lib().oev_table(ptr(t), N, ptr(cdf)) == 0
    return cdf


def sample_at(texels, Ke, p, n, wo, seed, *, type=1, albedo=(0.5, 0.5, 0.5), roughness=1.0, mis=False, last=True):
    """(reason R_*, c float32 [3], texel) of one environment sample at the vertex (p, n, wo) of a material, in an empty scene"""
    t = texels4(texels)
    N, ec = size_of(t), table(t)
    v = [np.asarray(a, np.float32) for a in (albedo, p, n, wo)]
    c, texel = np.zeros(3, np.float32), np.zeros(1, np.int32)
    why = lib().oev_sample_at(ptr(t), ptr(ec), N, Ke, int(mis), int(last), int(type), ptr(v[0]), float(roughness), ptr(v[1]), ptr(v[2]), ptr(v[3]),
                              int(seed), ptr(c), ptr(texel))
    assert why >= 0
    return why, c, int(texel[0])


def _inputs(tris, mats, lights, texels, env_cdf):
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    li = direct_oracle._lights(tris, mats, lights)
    cn = light_counts(li, len(tris))
    cdf, tri_q = power_oracle.table(tris, mats, li)
    t = texels4(texels)
    return tris, mats, li, cn, cdf, tri_q, t, size_of(t), (table(t) if env_cdf is None else np.ascontiguousarray(env_cdf, np.uint64))


def render(tris, mats, texels, W, H, frame_begin, frame_count, K, Ke, *, B=None, R=NEVER, cap=1.0, lights=None, env_cdf=None, cam=None,
           stripe_rows=1, n_ranks=1, rank=0, start=None):
    """float32 [local pixels, 4]: the framebuffer of pt_render_direct_env (``B`` None) or of pt_render_indirect_env with max_bounces ``B``
    and the roulette (``R``, ``cap``), with ``Ke`` environment samples, in ``roulette_oracle.render``'s layout."""
    tris, mats, li, cn, cdf, tri_q, t, N, ec = _inputs(tris, mats, lights, texels, env_cdf)
    rows = direct_oracle.local_row_count(H, stripe_rows, n_ranks, rank)
    fb = np.zeros((rows * W, 4), np.float32) if start is None else np.array(start, np.float32).reshape(rows * W, 4).copy()
    c = cam10(cam)
    rc = lib().oev_render(int(B is not None), _p(tris), len(tris), ptr(mats), _p(li), len(li), ptr(cdf), _p(tri_q), _p(cn), ptr(t), ptr(ec), N, Ke,
                          ptr(c), W, H, stripe_rows, n_ranks, rank, frame_begin, frame_count, K, B or 1, R, cap, ptr(fb))
    if rc == -2:
        raise ValueError("oev_render: the map or env_samples out of range")
    return None if rc != 0 else fb


def samples(tris, mats, texels, W, H, gid, frame, K, Ke, *, B=None, R=NEVER, cap=1.0, lights=None, env_cdf=None, cam=None, details=False):
    """Per sample (gid[i], frame[i]): radiance float32 [n, 3] before the fold; with ``details`` (radiance, dict) where the dict holds, for
    the first V = 1 (direct) or min(B, DETAIL_VERTICES) vertices: reason uint8 [n, V, Ke] (R_*) and texel int32 [n, V, Ke] of each
    environment sample, miss_texel int32 [n, V] (the texel of the ray that left the scene at that vertex, -1: none) and miss_wb float32
    [n, V] (its weight)."""
    tris, mats, li, cn, cdf, tri_q, t, N, ec = _inputs(tris, mats, lights, texels, env_cdf)
    gid = np.ascontiguousarray(gid, np.int32)
    frame = np.ascontiguousarray(frame, np.int32)
    n, Vn = len(gid), 1 if B is None else min(B, DETAIL_VERTICES)
    rad = np.zeros((n, 3), np.float32)
    d = dict(reason=np.zeros((n, Vn, Ke), np.uint8), texel=np.zeros((n, Vn, Ke), np.int32), miss_texel=np.zeros((n, Vn), np.int32),
             miss_wb=np.zeros((n, Vn), np.float32))
    c = cam10(cam)
    dp = tuple(ptr(d[k]) for k in ("reason", "texel", "miss_texel", "miss_wb")) if details else (None,) * 4
    rc = lib().oev_samples(int(B is not None), _p(tris), len(tris), ptr(mats), _p(li), len(li), ptr(cdf), _p(tri_q), _p(cn), ptr(t), ptr(ec), N, Ke,
                           ptr(c), W, H, ptr(gid), ptr(frame), n, K, B or 1, R, cap, ptr(rad), *dp)
    if rc != 0:
        raise ValueError("oev_samples rejected the camera, the map or env_samples")
    return (rad, d) if details else rad


THREADS = max(1, min(16, os.cpu_count() or 1))


def sample_frames(tris, mats, texels, W, H, frames, K, Ke, *, B=None, R=NEVER, cap=1.0, lights=None, cam=None, frame_begin=0, pixels=None):
    """radiance float64 [frames, pixels, 3] of every sample of frames [frame_begin, frame_begin + frames) -- of all W * H pixels, or of the
    global ids ``pixels`` --, computed in slices on threads (the library holds no state): the result is that of one call."""
    lib()
    t = texels4(texels)
    ec = table(t)
    px = np.arange(W * H, dtype=np.int32) if pixels is None else np.asarray(pixels, np.int32)

    def run(span):
        nf = span[1] - span[0]
        gid = np.tile(px, nf)
        frame = np.repeat(np.arange(span[0], span[1], dtype=np.int32), len(px))
        return samples(tris, mats, t, W, H, gid, frame, K, Ke, B=B, R=R, cap=cap, lights=lights, env_cdf=ec, cam=cam)

    step = max(1, -(-frames // (4 * THREADS)))
    spans = [(f, min(f + step, frame_begin + frames)) for f in range(frame_begin, frame_begin + frames, step)]
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(run, spans))
    return np.concatenate(parts).astype(np.float64).reshape(frames, len(px), 3)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
