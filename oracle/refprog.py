"""ctypes binding of the reference kernel's own program text, compiled for the host (oracle/_ref/libgencolors_ref.so: oracle/Makefile,
target `ref`; oracle/ref_glue.cl has the entry points, oracle/ref_builtins.cpp the OpenCL built-ins under PTSPEC), and of the oracle's
entry points that answer them one by one.

TEST INFRASTRUCTURE.  The library exists only where the reference checkout does (``available()``); it is never committed.  The
reference is fixed at 36 triangles (NUM_TRIANGLES) and 16 bounces: ``pad36`` brings a smaller scene there.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from oracle import ptoracle

_HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_DIR = os.environ.get("PT_REFERENCE_DIR", "/root/reference")
NUM_TRIANGLES = 36
BOUNCES = 16

_V, _I, _L, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
_REF_SIGNATURES = {
    "ref_hash": [_V, _V, _L],
    "ref_random": [_V, _V, _V, _L],
    "ref_get_ray": [_V, _V, _V, _L],
    "ref_generate_ray": [_V, _V, _I, _I, _V, _V, _V, _L],
    "ref_intersect_triangle": [_V, _V, _V, _V, _V, _V, _V, _L],
    "ref_intersect_world": [_V, _V, _V, _V, _V, _V, _L],
    "ref_reflect": [_V, _V, _V, _L],
    "ref_sample_hemisphere_cosine": [_V, _V, _V, _V, _L],
    "ref_sample_ggx": [_V, _V, _V, _V, _V, _V, _L],
    "ref_distribution_ggx": [_V, _V, _V, _L],
    "ref_brdf": [_V, _V, _V, _V, _V, _V, _V, _V, _V, _L],
    "ref_trace_rays": [_V, _V, _V, _V, _V, _V, _V, _L],
    "ref_gamma_correct": [_V, _V, _L],
    "ref_read_from_gamma": [_V, _V, _L],
    "ref_kernel": [_V, _V, _V, _I, _I, _I, _I, _U64],
    "ref_render": [_V, _V, _V, _I, _I, _I, _I],
}
_ORACLE_SIGNATURES = {
    "ptor_kat_hash_array": [_V, _V, _L],
    "ptor_kat_random_array": [_V, _V, _V, _L],
    "ptor_kat_get_ray": [_V, _V, _V, _L],
    "ptor_kat_intersect_triangle": [_V, _V, _V, _V, _V, _V, _V, _L],
    "ptor_kat_reflect": [_V, _V, _V, _L],
    "ptor_kat_sample_hemisphere_cosine": [_V, _V, _V, _V, _L],
    "ptor_kat_sample_ggx": [_V, _V, _V, _V, _V, _V, _L],
    "ptor_kat_distribution_ggx": [_V, _V, _V, _L],
    "ptor_kat_brdf": [_V, _V, _V, _V, _V, _V, _V, _V, _V, _L],
    "ptor_kat_trace_rays": [_V, _I, _V, _V, _V, _V, _I, _V, _V, _L],
}
_libs = {}
_bound = set()


def reference_present() -> bool:
    """whether the reference checkout is on this machine: where it is, a missing library is an error, not a reason to skip"""
    return os.path.isfile(os.path.join(REFERENCE_DIR, "test", "ClKernels", "GenerateColors.cl"))


def lib_path(variant: str = "") -> str:
    return os.path.join(_HERE, "_ref", "libgencolors_ref%s.so" % ("_" + variant if variant else ""))


def available(variant: str = "") -> bool:
    return os.path.exists(lib_path(variant))


def lib(variant: str = ""):
    """The compiled reference ("") or the same text over dot / cross without fused multiply-add ("nofma")."""
    if variant not in _libs:
        L = ctypes.CDLL(lib_path(variant))
        for name, args in _REF_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = None, args
        _libs[variant] = L
    return _libs[variant]


def oracle_lib(variant: str = ""):
    L = ptoracle.lib(variant)
    if variant not in _bound:
        for name, args in _ORACLE_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = None, args
        _bound.add(variant)
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f(a, cols=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if cols is None else a.reshape(-1, cols)


def _u(a):
    return np.ascontiguousarray(a, np.uint32).reshape(-1)


def _i(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def pad36(tris):
    """``tris`` followed by zero-area triangles (all vertices 0, material 0) up to the reference's 36: none of them can be hit,
    since det == 0 fails the reference's first test"""
    assert len(tris) <= NUM_TRIANGLES
    out = np.zeros(NUM_TRIANGLES, tris.dtype)
    out[: len(tris)] = tris
    return out


class Side:
    """One side of the comparison: the compiled reference (``Side("ref")``) or the oracle (``Side("oracle")``), each function of
    the reference's file under one name, on arrays of n records.  The oracle's values have three lanes where the reference's have
    four; the fourth is returned as None."""

    def __init__(self, which: str, variant: str = ""):
        assert which in ("ref", "oracle")
        self.ref = which == "ref"
        self.variant = variant
        self.L = lib(variant) if self.ref else oracle_lib(variant)

    def hash(self, x):
        x = _u(x)
        out = np.empty_like(x)
        (self.L.ref_hash if self.ref else self.L.ptor_kat_hash_array)(_p(x), _p(out), x.size)
        return out

    def random(self, seed):
        """(seed after, value)"""
        seed = _u(seed)
        after, val = np.empty_like(seed), np.empty(seed.size, np.float32)
        (self.L.ref_random if self.ref else self.L.ptor_kat_random_array)(_p(seed), _p(after), _p(val), seed.size)
        return after, val

    def get_ray(self, origin, direction):
        """(origin, dir) [n, 3] each; the reference's side adds invDir [n, 3] and sign [n, 3]"""
        o, d = _f(origin, 3), _f(direction, 3)
        if self.ref:
            out = np.empty((len(o), 12), np.float32)
            self.L.ref_get_ray(_p(o), _p(d), _p(out), len(o))
            return out[:, :3], out[:, 3:6], out[:, 6:9], out[:, 9:12]
        out = np.empty((len(o), 6), np.float32)
        self.L.ptor_kat_get_ray(_p(o), _p(d), _p(out), len(o))
        return out[:, :3], out[:, 3:6]

    def generate_ray(self, xc, yc, W, H, seed):
        """(origin [n, 3], dir [n, 3], seed after)"""
        xc, yc, seed = _i(xc), _i(yc), _u(seed)
        out, after = np.empty((xc.size, 6), np.float32), np.empty_like(seed)
        if self.ref:
            self.L.ref_generate_ray(_p(xc), _p(yc), W, H, _p(seed), _p(out), _p(after), xc.size)
        else:
            for k in range(xc.size):
                s = ctypes.c_uint32(int(seed[k]))
                o6 = np.empty(6, np.float32)
                self.L.ptor_kat_generate_ray(int(xc[k]), int(yc[k]), W, H, ctypes.byref(s), _p(o6))
                out[k], after[k] = o6, s.value
        return out[:, :3], out[:, 3:], after

    def intersect_triangle(self, tris, tri, origin, direction, tmax):
        """(accepted [n] bool, t [n], p [n, 3], n [n, 3]); zeros where not accepted"""
        tris, tri, o, d, tmax = np.ascontiguousarray(tris), _i(tri), _f(origin, 3), _f(direction, 3), _f(tmax).reshape(-1)
        out, hit = np.empty((len(o), 7), np.float32), np.empty(len(o), np.int32)
        (self.L.ref_intersect_triangle if self.ref else self.L.ptor_kat_intersect_triangle)(
            _p(tris), _p(tri), _p(o), _p(d), _p(tmax), _p(out), _p(hit), len(o))
        return hit != 0, out[:, 0], out[:, 1:4], out[:, 4:7]

    def intersect_world(self, tris, origin, direction):
        """(hit [n] bool, t [n], p [n, 3], n [n, 3], triangle [n], -1 without a hit); zeros without a hit"""
        tris, o, d = np.ascontiguousarray(tris), _f(origin, 3), _f(direction, 3)
        assert len(tris) == NUM_TRIANGLES or not self.ref
        out, hit, tri = np.zeros((len(o), 7), np.float32), np.empty(len(o), np.int32), np.empty(len(o), np.int32)
        if self.ref:
            self.L.ref_intersect_world(_p(tris), _p(o), _p(d), _p(out), _p(tri), _p(hit), len(o))
        else:
            t1 = ctypes.c_int(-1)
            for k in range(len(o)):
                hit[k] = self.L.ptor_kat_intersect_world(_p(tris), len(tris), _p(o[k]), _p(d[k]), _p(out[k]), ctypes.byref(t1))
                tri[k] = t1.value
        return hit != 0, out[:, 0], out[:, 1:4], out[:, 4:7], tri

    def reflect(self, v, n):
        v, n = _f(v, 3), _f(n, 3)
        out = np.empty_like(v)
        (self.L.ref_reflect if self.ref else self.L.ptor_kat_reflect)(_p(v), _p(n), _p(out), len(v))
        return out

    def sample_hemisphere_cosine(self, n, seed):
        """(wi [n, 3], seed after)"""
        n, seed = _f(n, 3), _u(seed)
        out, after = np.empty_like(n), np.empty_like(seed)
        (self.L.ref_sample_hemisphere_cosine if self.ref else self.L.ptor_kat_sample_hemisphere_cosine)(
            _p(n), _p(seed), _p(out), _p(after), len(n))
        return out, after

    def sample_ggx(self, n, roughness, seed):
        """(wh [n, 3], cosTheta [n], seed after)"""
        n, r, seed = _f(n, 3), _f(roughness).reshape(-1), _u(seed)
        out, ct, after = np.empty_like(n), np.empty_like(r), np.empty_like(seed)
        (self.L.ref_sample_ggx if self.ref else self.L.ptor_kat_sample_ggx)(_p(n), _p(r), _p(seed), _p(out), _p(ct), _p(after), len(n))
        return out, ct, after

    def distribution_ggx(self, cos_theta, roughness):
        c, r = _f(cos_theta).reshape(-1), _f(roughness).reshape(-1)
        out = np.empty_like(c)
        (self.L.ref_distribution_ggx if self.ref else self.L.ptor_kat_distribution_ggx)(_p(c), _p(r), _p(out), c.size)
        return out

    def brdf(self, wo, normal, mats, mat_index, seed, wi_before, pdf_before):
        """(colour [n, 3], colour's fourth lane or None, wi [n, 3], pdf [n], seed after)"""
        wo, normal, mats, mi, seed = _f(wo, 3), _f(normal, 3), np.ascontiguousarray(mats), _i(mat_index), _u(seed)
        wi, pdf, after = _f(wi_before, 3).copy(), _f(pdf_before).reshape(-1).copy(), np.empty_like(seed)
        col = np.empty((len(wo), 4 if self.ref else 3), np.float32)
        (self.L.ref_brdf if self.ref else self.L.ptor_kat_brdf)(
            _p(wo), _p(normal), _p(mats), _p(mi), _p(seed), _p(col), _p(wi), _p(pdf), _p(after), len(wo))
        return col[:, :3], (col[:, 3] if self.ref else None), wi, pdf, after

    def trace_rays(self, tris, mats, origin, direction, seed):
        """(radiance [n, 3], seed after) of 16 bounces from the rays as given"""
        tris, mats, o, d, seed = np.ascontiguousarray(tris), np.ascontiguousarray(mats), _f(origin, 3), _f(direction, 3), _u(seed)
        assert len(tris) == NUM_TRIANGLES or not self.ref
        after = np.empty_like(seed)
        if self.ref:
            out = np.empty((len(o), 4), np.float32)
            self.L.ref_trace_rays(_p(tris), _p(mats), _p(o), _p(d), _p(seed), _p(out), _p(after), len(o))
        else:
            out = np.empty((len(o), 3), np.float32)
            self.L.ptor_kat_trace_rays(_p(tris), len(tris), _p(mats), _p(o), _p(d), _p(seed), BOUNCES, _p(out), _p(after), len(o))
        return out[:, :3], after

    def render(self, tris, mats, W, H, frames, frame_begin=0, fb=None):
        """frames [frame_begin, frame_begin + frames) over all pixels: the [W * H, 4] framebuffer (``fb``, updated in place, or a new
        one of zeros)"""
        tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
        assert len(tris) == NUM_TRIANGLES or not self.ref
        if not self.ref:
            return ptoracle.render(tris, mats, W, H, frames, frame_begin=frame_begin, fb=fb, variant=self.variant)
        if fb is None:
            fb = np.zeros((W * H, 4), np.float32)
        assert fb.dtype == np.float32 and fb.size == W * H * 4 and fb.flags.c_contiguous
        self.L.ref_render(_p(tris), _p(mats), _p(fb), W, H, frame_begin, frames)
        return fb


def gamma(which: str, value4):
    """gammaCorrect ("correct") or readFromGamma ("read") of [n, 4] values, by the compiled reference"""
    v = _f(value4, 4)
    out = np.empty_like(v)
    (lib().ref_gamma_correct if which == "correct" else lib().ref_read_from_gamma)(_p(v), _p(out), len(v))
    return out


def kernel(tris, mats, fb, W, H, z, gid, w=0):
    """one invocation of the reference's kernel as work-item ``gid`` with cRes = (W, H, z, w), on ``fb`` in place"""
    tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
    assert len(tris) == NUM_TRIANGLES and fb.dtype == np.float32 and fb.flags.c_contiguous and fb.size >= 4 * W * H and 0 <= gid < W * H
    lib().ref_kernel(_p(tris), _p(mats), _p(fb), W, H, z, w, gid)
