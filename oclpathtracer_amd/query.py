"""Batched ray queries: the renderer's closest-hit search for rays of the caller's (``pt_intersect_rays``, ``pt_camera_rays``).

* ``RAY_DTYPE`` / ``HIT_DTYPE`` -- the 32-byte ``pt_ray`` and the 48-byte ``pt_hit`` of include/pt_shim.h as numpy records.
* ``make_rays``                -- a RAY_DTYPE array from origins, directions and tmax.
* ``RayCaster``                -- ``closest(rays)``, ``occluded(rays)`` and ``camera_rays(width, height, frame, camera)`` for one
  triangle buffer on one device.  Numpy in, numpy out (synchronous); or device torch tensors ``[N, 8]`` float32 in, device tensors
  out (``[N, 12]`` float32 -- int fields as their bits -- or ``[N]`` int32) on the caster's GPU, used in place and ordered against
  torch's current stream by device-side waits, without a host sync: a tensor is reached through a wrap of its address range
  (``pt_buffer_wrap``), kept for whatever tensor occupies that range later, and the tensor itself is not held.

A ray's direction may have any length: it is normalised on the device exactly as the reference's getRay does, and t is a
distance along the normalised direction.  A hit counts at 0 < t < min(tmax, 1e20).  All compute is HIP in libptshim.so; nothing
here has a CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import adl, scene, shim
from .camera import Camera

RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("tmax", "<f4"), ("dir", "<f4", (3,)), ("reserved", "<i4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("tri", "<i4"), ("u", "<f4"), ("v", "<f4"), ("p", "<f4", (3,)), ("material", "<i4"),
                      ("n", "<f4", (3,)), ("reserved", "<i4")])
assert RAY_DTYPE.itemsize == ctypes.sizeof(shim.Ray) == 32 and HIT_DTYPE.itemsize == ctypes.sizeof(shim.Hit) == 48

RAY_WORDS, HIT_WORDS = 8, 12   # float32 words per record: the torch layouts [N, 8] and [N, 12]
# Address ranges of caller tensors kept wrapped.  Freeing a wrap waits for the device (pt_buffer_free), so the tensor path never
# frees one: torch's caching allocator hands the same blocks back, and a wrap is reused for whatever tensor occupies its range.
# Wraps beyond this many are freed only where the caster waits for the device anyway (the numpy path) and at release().
_WRAP_KEEP = 64
_EARLY_EXIT = -1   # RayCaster._query: occlusion by pt_occluded_rays (not a pt_intersect_rays mode)


def make_rays(origins, dirs, tmax=1e20) -> np.ndarray:
    """A RAY_DTYPE array of len(origins) rays; ``tmax`` is a scalar or one value per ray."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape")
    r = np.zeros(len(o), RAY_DTYPE)
    r["origin"], r["dir"] = o, d
    r["tmax"] = np.broadcast_to(np.asarray(tmax, np.float32), (len(o),))
    return r


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch")


# ---- argument checks (before anything is enqueued) --------------------------------------------------------------------
def check_numpy_rays(rays) -> np.ndarray:
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE and a.ndim == 1:
        return np.ascontiguousarray(a)
    if a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == RAY_WORDS:
        return np.ascontiguousarray(a).view(RAY_DTYPE).reshape(-1)
    raise TypeError("rays must be a RAY_DTYPE array or float32 [N, 8]; got %s %s" % (a.dtype, a.shape))


def check_tensor_rays(t, dev: adl.Device) -> None:
    import torch

    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != RAY_WORDS:
        raise TypeError("ray tensors must be float32 [N, 8]; got %s %s" % (t.dtype, tuple(t.shape)))
    if not t.is_cuda:
        raise ValueError("ray tensors must live on the device")
    if t.device.index != dev.m_deviceIdx:
        raise ValueError("ray tensor on %s, the caster's device is cuda:%d" % (t.device, dev.m_deviceIdx))
    if not t.is_contiguous():
        raise ValueError("ray tensors must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError("ray tensors must be 16-byte aligned")


class DeviceIO:
    """How a caster's arguments and results reach the device: staging buffers for numpy arrays, grown on demand, and for torch
    tensors wraps of their address ranges, kept (see ``_WRAP_KEEP``), with the one event that orders a call against torch's stream."""

    def __init__(self, dev: adl.Device):
        self.dev = dev
        self._host = {}    # role -> (adl.Buffer, capacity in bytes): device staging of the numpy path, grown on demand
        self._wrapped = {}  # (address, bytes) -> adl.Buffer: address ranges of caller tensors, wrapped with pt_buffer_wrap (oldest first)
        self._sync = None

    def staging(self, role: str, nbytes: int) -> adl.Buffer:
        buf, cap = self._host.get(role, (None, 0))
        if buf is None or cap < nbytes:
            if buf is not None:
                buf.release()
            cap = max(nbytes, 1 << 12)
            buf = adl.Buffer(self.dev, cap, np.uint8)
            self._host[role] = (buf, cap)
        return buf

    def wrap(self, t) -> adl.Buffer:
        """The wrap of t's address range (made once per range; never freed here: see _WRAP_KEEP)."""
        key = (int(t.data_ptr()), int(t.numel() * t.element_size()))
        b = self._wrapped.pop(key, None)
        if b is None:
            b = adl.Buffer()
            b.setRawPtr(self.dev, key[0], key[1])
        self._wrapped[key] = b   # (most recently used last)
        return b

    def trim_wraps(self) -> None:
        """Free the least recently used wraps beyond _WRAP_KEEP -- called only right after a wait for the device."""
        while len(self._wrapped) > _WRAP_KEEP:
            self._wrapped.pop(next(iter(self._wrapped))).release()

    def on_tensors(self, enqueue, *tensors) -> None:
        """``enqueue(*wraps, event handle)`` on the tensors' memory, behind what torch's current stream holds -- the arguments are
        written and the results' memory is free there -- and torch's later work behind the event: device-side waits only.  The wraps
        do not hold the tensors: their memory follows torch's stream rules."""
        import torch

        stream = torch.cuda.current_stream(tensors[0].device)
        wraps = [self.wrap(t) for t in tensors]
        if self._sync is None:
            self._sync = adl.SyncObject(self.dev)
        self.dev.waitStream(stream.cuda_stream)
        enqueue(*wraps, self._sync._h)
        self._sync.waitOnStream(stream.cuda_stream)

    def release(self) -> None:
        for b in [b for b, _ in self._host.values()] + list(self._wrapped.values()):
            b.release()
        self._host.clear()
        self._wrapped.clear()
        if self._sync is not None:
            self._sync.release()
            self._sync = None


def into_tensor(dev: adl.Device, out, sync: Optional[adl.SyncObject], enqueue) -> adl.SyncObject:
    """One result into a tensor of the caller's: ``enqueue(handle of out's memory, event handle)`` behind torch's current stream,
    and torch's later work behind the event (``sync``, made here when None, and returned).  Unlike a caster's, the wrap is not
    kept: it is released here, which waits for the device -- the tensor is complete when this returns."""
    import torch

    stream = torch.cuda.current_stream(out.device)
    wrap = adl.Buffer()
    wrap.setRawPtr(dev, int(out.data_ptr()), int(out.numel() * out.element_size()))
    if sync is None:
        sync = adl.SyncObject(dev)
    try:
        dev.waitStream(stream.cuda_stream)
        enqueue(wrap._h, sync._h)
        sync.waitOnStream(stream.cuda_stream)
    finally:
        wrap.release()
    return sync


class RayCaster(scene.SceneHolder):
    """Closest-hit and occlusion queries against ``triangles`` on ``dev``.

    ``triangles``: a ``scene.TRIANGLE_DTYPE`` array (uploaded to a buffer of this caster's), or an ``adl.Buffer`` that already
    holds them -- the renderer's own (``Renderer.ray_caster``), so that queries and renders share one prepared scene and one LBVH
    (``num_triangles`` then says how many records count).  The search follows the device's options exactly as renders do."""

    def __init__(self, dev: adl.Device, triangles, *, num_triangles: Optional[int] = None):
        self.dev = dev
        self._lib = shim.load()
        self.scene = scene.SceneBuffers(dev, triangles, num_triangles, shape="triangles")
        self._io = DeviceIO(dev)

    # ---- queries ------------------------------------------------------------------------------------------------------
    def closest(self, rays):
        """The reference's closest hit of every ray: a HIT_DTYPE array (numpy rays) or a float32 [N, 12] device tensor (tensor
        rays; view it as int32 for tri and material)."""
        return self._query(rays, shim.PT_QUERY_CLOSEST)

    def occluded(self, rays, early_exit: bool = False):
        """1 where the ray hits some triangle at 0 < t < min(tmax, 1e20), else 0: int32 [N], numpy or a device tensor.
        ``early_exit``: the search stops at the first triangle accepted below the limit (``pt_occluded_rays``); the result is the
        same array."""
        if not isinstance(early_exit, bool):
            raise TypeError("early_exit must be a bool")
        return self._query(rays, _EARLY_EXIT if early_exit else shim.PT_QUERY_OCCLUDED)

    def _launch(self, rb, ob, n: int, mode: int, ev) -> None:
        if mode == _EARLY_EXIT:
            shim.check(self._lib.pt_occluded_rays(self.dev._h, self.tbuf._h, self.num_triangles, rb._h, ob._h, n, ev))
        else:
            shim.check(self._lib.pt_intersect_rays(self.dev._h, self.tbuf._h, self.num_triangles, rb._h, ob._h, n, mode, ev))

    def _query(self, rays, mode: int):
        if _is_tensor(rays):
            return self._query_tensor(rays, mode)
        r = check_numpy_rays(rays)
        n = len(r)
        out = np.zeros(n, HIT_DTYPE) if mode == shim.PT_QUERY_CLOSEST else np.zeros(n, np.int32)
        rb = self._io.staging("rays", r.nbytes)
        ob = self._io.staging("out", out.nbytes)
        if n:
            rb.write(r.view(np.uint8), r.nbytes)
        self._launch(rb, ob, n, mode, None)
        if n:
            ob.read(out.view(np.uint8), out.nbytes)
        self.dev.waitForCompletion()
        self._io.trim_wraps()
        return out

    def _query_tensor(self, rays, mode: int):
        import torch

        check_tensor_rays(rays, self.dev)
        n = rays.shape[0]
        shape = (n, HIT_WORDS) if mode == shim.PT_QUERY_CLOSEST else (n,)
        out = torch.empty(shape, dtype=torch.float32 if mode == shim.PT_QUERY_CLOSEST else torch.int32, device=rays.device)
        if n == 0:
            return out
        rays.record_stream(torch.cuda.current_stream(rays.device))
        self._io.on_tensors(lambda rb, ob, ev: self._launch(rb, ob, n, mode, ev), rays, out)
        return out

    def camera_rays(self, width: int, height: int, frame: int, camera: Optional[Camera] = None, *, as_tensor: bool = False):
        """The renderer's primary rays of ``frame`` seen from ``camera`` (None: the reference's): ray y * width + x is pixel (x, y).
        Their directions are the vectors the reference hands to getRay (normalised once), so ``closest(camera_rays(...))``
        traces the renderer's first bounce bit for bit.  A RAY_DTYPE array, or a float32 [width * height, 8] device tensor."""
        width, height, frame = int(width), int(height), int(frame)
        if width < 1 or height < 1 or frame < 0:
            raise ValueError("invalid image geometry or frame")
        struct = Camera.struct_of(camera)
        cam = ctypes.byref(struct) if struct is not None else None
        n = width * height
        if as_tensor:
            import torch

            out = torch.empty((n, RAY_WORDS), dtype=torch.float32, device="cuda:%d" % self.dev.m_deviceIdx)
            self._io.on_tensors(lambda ob, ev: shim.check(self._lib.pt_camera_rays(self.dev._h, cam, width, height, frame, ob._h, ev)), out)
            return out
        out = np.zeros(n, RAY_DTYPE)
        ob = self._io.staging("camera", out.nbytes)
        shim.check(self._lib.pt_camera_rays(self.dev._h, cam, width, height, frame, ob._h, None))
        ob.read(out.view(np.uint8), out.nbytes)
        self.dev.waitForCompletion()
        self._io.trim_wraps()
        return out

    def release(self) -> None:
        self._io.release()
        self.scene.release()
