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

from . import adl, image, scene, shim
from .camera import Camera
from .image import LIMIT, ImageRenderer, ImageShare, frame_range
from .query import into_tensor
from .shim import MOMENTS_DTYPE

FEATURES = ("albedo", "normal", "depth", "emission")   # the order of pt_render_features' outputs
_WORKSPACE_BYTES = 64 << 20   # the default workspaces hold, all together, as many whole frames as fit in this, at most 64


def variance_map(r, mom: adl.Buffer, valid: bool, noise_map: Optional[adl.Buffer], idle_wait: bool = False):
    """``(var float32 [local_pixels, 3], n uint32 [local_pixels], the noise map)`` of renderer ``r``'s moments ``mom``: resolved on the
    device (``pt_moments_resolve``) into ``noise_map`` (made here on first use), read back and split; synchronises.  Zeros while the
    moments are not ``valid``, without a device call -- but for a wait where the caller has always waited (``idle_wait``)."""
    rec = np.zeros((r.local_pixels, 4), np.float32)
    if r.local_pixels and valid:
        if noise_map is None:
            noise_map = adl.Buffer(r.dev, r.local_pixels, adl.float4)
        shim.check(r._lib.pt_moments_resolve(r.dev._h, mom._h, r.local_pixels, noise_map._h, None, None))
        noise_map.read(rec, r.local_pixels)
        r.dev.waitForCompletion()
    elif idle_wait:
        r.dev.waitForCompletion()
    return np.ascontiguousarray(rec[:, :3]), np.ascontiguousarray(rec[:, 3]).view(np.uint32), noise_map


class FeatureRenderer(ImageRenderer, scene.SceneHolder):
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
        ImageShare.__init__(self, width, height, stripe_rows, n_ranks, rank)
        if workspace_frames is not None and int(workspace_frames) < 1:
            raise ValueError("workspace_frames must be at least 1")
        self._set_camera(camera)
        self._noise = self._sync = None
        self.samples, self.mom = {}, {}
        self.scene = scene.SceneBuffers(dev, triangles, num_triangles, materials, num_materials, shape="materials")
        n = max(self.local_pixels, 1)
        if workspace_frames is None:
            workspace_frames = max(1, min(64, _WORKSPACE_BYTES // (12 * n * len(self.features))))
        self.workspace_frames = min(int(workspace_frames), max(1, LIMIT // n))   # (a call is one launch: fewer than 2^31 samples)
        self.frames_done = 0
        self._valid = False   # the moments hold this image's sums (a call from frame 0 has reset them)
        try:
            for f in self.features:
                self.samples[f] = adl.Buffer(dev, 3 * n * self.workspace_frames, np.float32)
                self.mom[f] = adl.Buffer(dev, n * MOMENTS_DTYPE.itemsize, np.uint8)
        except Exception:
            self.release()
            raise

    @classmethod
    def on(cls, renderer, **kw) -> "FeatureRenderer":
        """A feature renderer on ``renderer``'s scene buffers (``Renderer.feature_renderer``, ``DirectRenderer.denoiser`` and
        ``.temporal``): one prepared scene, one LBVH.  ``kw`` are this class's; the image size, camera and sharding default to
        ``renderer``'s.  Release it before the renderer."""
        width, height = image.like(renderer, kw)
        return cls(renderer.dev, renderer.tbuf, renderer.mbuf, width, height, num_triangles=renderer.num_triangles,
                   num_materials=renderer.num_materials, **kw)

    def _restart(self) -> None:
        self.frames_done = 0
        self._valid = False

    def params(self, frames: int, frame_begin: int) -> shim.FeatureParams:
        p = self.fill(shim.FeatureParams(), frames, frame_begin)
        p.num_triangles, p.num_materials = self.num_triangles, self.num_materials
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
        frames, frame_begin = frame_range(frames, frame_begin, self.frames_done, resumes=not restart)
        outs = [adl._handle(self.samples.get(f)) for f in FEATURES]
        first, end = frame_begin, frame_begin + frames
        while first < end:
            k = min(self.workspace_frames, end - first)
            p = self.params(k, first)
            shim.check(self._lib.pt_render_features(self.dev._h, self.tbuf._h, self.mbuf._h, *outs, ctypes.byref(p), self._cam_ref(), None))
            last = first + k == end
            for i, f in enumerate(self.features):
                ev = adl._handle(sync) if last and i == len(self.features) - 1 else None
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
                self._sync = into_tensor(self.dev, out, self._sync, lambda out_h, ev: shim.check(
                    self._lib.pt_moments_resolve(self.dev._h, self.mom[name]._h, self.local_pixels, out_h, None, ev)))
            return out
        var, n, self._noise = variance_map(self, self.mom[name], self._valid, self._noise, idle_wait=True)
        return var, n

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
        self.scene.release()
