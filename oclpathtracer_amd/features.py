"""First-hit feature buffers on the device (``pt_render_features``): what a denoiser, a compositor or a model takes beside the noisy
image -- per-pixel albedo, shading normal, depth / coverage and emission at the first hit, averaged over the same jittered (and, with a
lens, defocused) samples the lit renderers take, with their variances.

A sample of a pixel traces the renderer's primary ray -- direct illumination's steps 1 and 2 and nothing after them.  On a hit it
records the material's albedo as stored, the normal turned to face the ray, ``(t, 1, -dot(n, d))`` and the emission; a miss records
zeros.  The second channel of ``depth`` is the coverage weight: the mean depth over a pixel's hits is sum[0] / sum[1].  Every feature's
samples go through ``pt_sample_moments`` on the device, frames ascending, so a pixel's sums, mean and variance are those of all its
frames.  Nothing is filtered here: the moments are what ``denoise.Denoiser`` (``pt_denoise``) takes as the guides of its filter.
``include/pt_shim.h`` states every expression.  All compute is HIP in libptshim.so; nothing here has a CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import adl, scene, shim
from .camera import Camera

FEATURES = ("albedo", "normal", "depth", "emission")   # the order of pt_render_features' outputs
MOMENTS_DTYPE = np.dtype([("sum", np.float64, 3), ("sum2", np.float64, 3), ("n", np.uint32), ("rejected", np.uint32)])   # pt_pixel_moments
assert MOMENTS_DTYPE.itemsize == ctypes.sizeof(shim.PixelMoments) == 56
_WORKSPACE_BYTES = 64 << 20   # the default workspaces hold, all together, as many whole frames as fit in this, at most 64


class FeatureRenderer:
    """First-hit features of a ``width`` x ``height`` image of ``triangles`` with ``materials`` on ``dev``.

    ``triangles`` / ``materials``: ``scene.TRIANGLE_DTYPE`` / ``scene.MATERIAL_DTYPE`` arrays (uploaded to buffers of this renderer's),
    or ``adl.Buffer``s that already hold them -- a renderer's own (``Renderer.feature_renderer``), so that both share one prepared
    scene and one LBVH (``num_triangles`` / ``num_materials`` then say how many records count).  ``features``: which of ``FEATURES``
    to keep; the others are neither computed nor stored.  ``workspace_frames`` sizes the sample workspaces: that many frames are written
    by one call and taken into the moments by the next.  ``stripe_rows`` / ``n_ranks`` / ``rank`` select the rows this device owns, as
    for ``Renderer``.  The search follows the device's options exactly as renders do."""

    def __init__(self, dev: adl.Device, triangles, materials, width: int, height: int, *, features=("albedo", "normal", "depth"),
                 camera: Optional[Camera] = None, num_triangles: Optional[int] = None, num_materials: Optional[int] = None,
                 stripe_rows: int = 16, n_ranks: int = 1, rank: int = 0, workspace_frames: Optional[int] = None):
        self.dev = dev
        self._lib = shim.load()
        self.features = tuple(features)
        if not self.features or len(set(self.features)) != len(self.features) or any(f not in FEATURES for f in self.features):
            raise ValueError("features must be a non-empty selection of %s without repeats" % (FEATURES,))
        self.width, self.height = int(width), int(height)
        self.stripe_rows, self.n_ranks, self.rank = int(stripe_rows), int(n_ranks), int(rank)
        if self.width < 1 or self.height < 1 or self.width * self.height > 0x7fffffff:
            raise ValueError("invalid image size %dx%d" % (self.width, self.height))
        if workspace_frames is not None and int(workspace_frames) < 1:
            raise ValueError("workspace_frames must be at least 1")
        self.local_rows = self._lib.pt_local_rows(self.height, self.stripe_rows, self.n_ranks, self.rank)
        if self.local_rows < 0:
            raise ValueError("invalid stripe geometry")
        self.local_pixels = self.local_rows * self.width
        self._set_camera(camera)
        self.tbuf = self.mbuf = self._noise = self._sync = None
        self._own_tbuf = self._own_mbuf = False
        self.samples, self.mom = {}, {}
        m_host = isinstance(materials, np.ndarray)
        if not (m_host or isinstance(materials, adl.Buffer)) or (m_host and materials.dtype != scene.MATERIAL_DTYPE):
            raise TypeError("materials must be a scene.MATERIAL_DTYPE array or an adl.Buffer")
        if not m_host and num_materials is None:
            raise ValueError("num_materials is required with an adl.Buffer of materials")
        self.num_materials = len(materials) if m_host else int(num_materials)
        if self.num_materials < 1:
            raise ValueError("a scene needs at least one material")
        n = max(self.local_pixels, 1)
        if workspace_frames is None:
            workspace_frames = max(1, min(64, _WORKSPACE_BYTES // (12 * n * len(self.features))))
        self.workspace_frames = min(int(workspace_frames), max(1, 0x7fffffff // n))   # (a call is one launch: fewer than 2^31 samples)
        self.frames_done = 0
        self._valid = False   # the moments hold this image's sums (a call from frame 0 has reset them)
        try:
            self.tbuf, self.num_triangles, self._own_tbuf = scene.triangle_buffer(dev, triangles, num_triangles)
            if m_host:
                self.mbuf, self._own_mbuf = adl.Buffer(dev, self.num_materials, scene.MATERIAL_DTYPE), True
                self.mbuf.write(np.ascontiguousarray(materials), self.num_materials)
            else:
                self.mbuf = materials
            for f in self.features:
                self.samples[f] = adl.Buffer(dev, 3 * n * self.workspace_frames, np.float32)
                self.mom[f] = adl.Buffer(dev, n * MOMENTS_DTYPE.itemsize, np.uint8)
        except Exception:
            self.release()
            raise

    def _set_camera(self, camera: Optional[Camera]) -> None:
        self._cam = Camera.struct_of(camera)   # rejected here, before anything is enqueued
        self.camera = camera

    def set_camera(self, camera: Optional[Camera]) -> None:
        """Features from ``camera``, its lens included, from now on (None: the reference's); the next render starts again at frame 0."""
        self._set_camera(camera)
        self.frames_done = 0
        self._valid = False

    def params(self, frames: int, frame_begin: int) -> shim.FeatureParams:
        p = shim.FeatureParams()
        p.width, p.height = self.width, self.height
        p.frame_begin, p.frame_count = frame_begin, frames
        p.num_triangles, p.num_materials = self.num_triangles, self.num_materials
        p.stripe_rows, p.n_ranks, p.rank = self.stripe_rows, self.n_ranks, self.rank
        return p

    def _need(self, name: str) -> None:
        if name not in self.samples:
            raise KeyError("this renderer keeps no %r: its features are %s" % (name, self.features))

    def render(self, frames: int, frame_begin: Optional[int] = None, sync: Optional[adl.SyncObject] = None, *, restart: bool = False) -> None:
        """Enqueue frames [frame_begin, frame_begin + frames) (default: continue after the last call) in calls of at most
        ``workspace_frames`` frames, each followed by the moments of every feature's samples; frame_begin 0 starts the moments afresh.
        frame_begin must be 0 or ``frames_done``: a frame rendered twice would be counted twice.  ``restart``: the moments start
        afresh at ANY frame_begin -- the image of a new camera whose frames go on where a lit renderer's stand
        (``temporal.TemporalAccumulator``)."""
        if frame_begin is None:
            frame_begin = self.frames_done
        frames, frame_begin = int(frames), int(frame_begin)
        if frames < 0 or frame_begin < 0 or frame_begin + frames > 0x7fffffff:
            raise ValueError("invalid frame range [%d, %d)" % (frame_begin, frame_begin + frames))
        if frames > 0 and not restart and frame_begin not in (0, self.frames_done):
            raise ValueError("a render starts at frame 0 or at frames_done (%d), not at %d" % (self.frames_done, frame_begin))
        cam = ctypes.byref(self._cam) if self._cam is not None else None
        outs = [self.samples[f]._h if f in self.samples else None for f in FEATURES]
        first, end = frame_begin, frame_begin + frames
        while first < end:
            k = min(self.workspace_frames, end - first)
            p = self.params(k, first)
            shim.check(self._lib.pt_render_features(self.dev._h, self.tbuf._h, self.mbuf._h, *outs, ctypes.byref(p), cam, None))
            last = first + k == end
            for i, f in enumerate(self.features):
                ev = sync._h if sync is not None and last and i == len(self.features) - 1 else None
                if self.local_pixels:
                    shim.check(self._lib.pt_sample_moments(self.dev._h, self.samples[f]._h, self.mom[f]._h, self.local_pixels, k,
                                                           int(first == 0 or (restart and first == frame_begin)), ev))
            first += k
        if frames > 0:
            self._valid = True
            self.frames_done = end

    def moments(self, name: str) -> np.ndarray:
        """``MOMENTS_DTYPE`` [local_pixels]: per channel the sum and the sum of squares of the feature's finite samples over every frame
        since the last start at frame 0, their number, and the samples rejected for a NaN or an infinity (synchronises)."""
        self._need(name)
        out = np.zeros(self.local_pixels, MOMENTS_DTYPE)
        if self.local_pixels and self._valid:
            self.mom[name].read(out.view(np.uint8), out.nbytes)
        self.dev.waitForCompletion()
        return out

    def mean(self, name: str) -> np.ndarray:
        """float64 [local_pixels, 3]: pt_moments_resolve's step 1 on the moments read back -- m = sum / n, 0 for a pixel without a
        finite sample (synchronises)."""
        m = self.moments(name)
        n = m["n"].astype(np.float64)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, m["sum"] / n, 0.0)

    def variance(self, name: str, *, as_tensor: bool = False):
        """The unbiased variance of one sample of the feature, resolved on the device (``pt_moments_resolve``): ``(var float32
        [local_pixels, 3], n uint32 [local_pixels])``, n the pixel's finite samples (a pixel with n < 2 has variance 0); synchronises.
        ``as_tensor``: a float32 [local_pixels, 4] tensor on the device instead -- the records as they are, var then n's bits --,
        ordered on torch's current stream, without a host wait."""
        self._need(name)
        if as_tensor:
            import torch

            out = torch.zeros((self.local_pixels, 4), dtype=torch.float32, device="cuda:%d" % self.dev.m_deviceIdx)
            if self.local_pixels and self._valid:
                self._resolve_into(name, out)
            return out
        rec = np.zeros((self.local_pixels, 4), np.float32)
        if self.local_pixels and self._valid:
            if self._noise is None:
                self._noise = adl.Buffer(self.dev, self.local_pixels, adl.float4)
            shim.check(self._lib.pt_moments_resolve(self.dev._h, self.mom[name]._h, self.local_pixels, self._noise._h, None, None))
            self._noise.read(rec, self.local_pixels)
        self.dev.waitForCompletion()
        return np.ascontiguousarray(rec[:, :3]), np.ascontiguousarray(rec[:, 3]).view(np.uint32)

    def _resolve_into(self, name: str, out) -> None:
        """pt_moments_resolve into a tensor of the caller's, as RayCaster writes into one: behind torch's stream, and torch's later
        work behind the result"""
        import torch

        stream = torch.cuda.current_stream(out.device)
        wrap = adl.Buffer()
        wrap.setRawPtr(self.dev, int(out.data_ptr()), int(out.numel() * out.element_size()))
        if self._sync is None:
            self._sync = adl.SyncObject(self.dev)
        try:
            self.dev.waitStream(stream.cuda_stream)
            shim.check(self._lib.pt_moments_resolve(self.dev._h, self.mom[name]._h, self.local_pixels, wrap._h, None, self._sync._h))
            self._sync.waitOnStream(stream.cuda_stream)
        finally:
            wrap.release()   # (waits for the device: the tensor is complete when this returns)

    def depth(self):
        """``(mean t over the pixel's hits float64 [local_pixels], coverage float64 [local_pixels])`` from the depth feature's sums:
        sum[0] / sum[1] (0 for a pixel never hit) and sum[1] / n (synchronises)."""
        m = self.moments("depth")
        s = m["sum"]
        n = m["n"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(s[:, 1] > 0, s[:, 0] / s[:, 1], 0.0), np.where(n > 0, s[:, 1] / n, 0.0)

    def read_samples(self, name: str, frames: Optional[int] = None) -> np.ndarray:
        """float32 [frames, local_pixels, 3]: the feature's samples of the last call's first ``frames`` frames, as the workspace holds
        them (default: the whole workspace; synchronises)."""
        self._need(name)
        k = self.workspace_frames if frames is None else int(frames)
        if not 0 <= k <= self.workspace_frames:
            raise ValueError("the workspace holds %d frames" % self.workspace_frames)
        out = np.zeros((k, self.local_pixels, 3), np.float32)
        if out.size:
            self.samples[name].read(out, out.size)
        self.dev.waitForCompletion()
        return out

    def release(self) -> None:
        for b in list(self.samples.values()) + list(self.mom.values()) + [self._noise, self._sync]:
            if b is not None:
                b.release()
        self.samples, self.mom = {}, {}
        self._noise = self._sync = None
        if self._own_tbuf and self.tbuf is not None:
            self.tbuf.release()
        if self._own_mbuf and self.mbuf is not None:
            self.mbuf.release()
        self.tbuf = self.mbuf = None
