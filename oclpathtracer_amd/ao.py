"""Ambient occlusion on the device (``pt_render_ao``): the AmbientOcclusion case the reference's harness declares, built from the
reference's own steps -- its RNG stream, camera, triangle test and cosine-weighted hemisphere sampling.

A sample of a pixel traces the renderer's primary ray; when it hits, ``rays_per_sample`` (K) occlusion rays leave the hit point
over the hemisphere of the normal that faces the ray, and an occlusion ray is *open* when no triangle lies at 0 < t < min(radius,
1e20) along it.  The device keeps per pixel the counts ``{open, hits}`` (uint32 each); the AO value is open / (K hits), or
``miss_value`` for a pixel none of whose samples hit the scene.  All compute is HIP in libptshim.so; nothing here has a CPU
fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import adl, scene, shim
from .camera import Camera
from .image import ImageRenderer, ImageShare, frame_range


class AORenderer(ImageRenderer, scene.SceneHolder):
    """Ambient occlusion of a ``width`` x ``height`` image of ``triangles`` on ``dev``.

    ``triangles``: a ``scene.TRIANGLE_DTYPE`` array (uploaded to a buffer of this renderer's), or an ``adl.Buffer`` that already
    holds them -- a renderer's own (``Renderer.ao_renderer``), so that both share one prepared scene and one LBVH
    (``num_triangles`` then says how many records count).  ``stripe_rows`` / ``n_ranks`` / ``rank`` select the rows this device
    owns, as for ``Renderer``.  The search follows the device's options exactly as renders do."""

    def __init__(self, dev: adl.Device, triangles, width: int, height: int, *, rays_per_sample: int = 16, radius: float = 1.0,
                 miss_value: float = 1.0, camera: Optional[Camera] = None, num_triangles: Optional[int] = None,
                 stripe_rows: int = 16, n_ranks: int = 1, rank: int = 0):
        self.dev = dev
        self._lib = shim.load()
        self.rays_per_sample, self.radius, self.miss_value = int(rays_per_sample), float(radius), float(miss_value)
        ImageShare.__init__(self, width, height, stripe_rows, n_ranks, rank)
        if not 1 <= self.rays_per_sample <= 256:
            raise ValueError("rays_per_sample must lie in 1..256")
        if not (math.isfinite(self.radius) and self.radius > 0.0):
            raise ValueError("radius must be finite and > 0")
        if not math.isfinite(self.miss_value):
            raise ValueError("miss_value must be finite")
        self._set_camera(camera)
        self.counts = self.image = None
        self.scene = scene.SceneBuffers(dev, triangles, num_triangles, shape="triangles")
        n = max(self.local_pixels, 1)
        try:
            self.counts = adl.Buffer(dev, 2 * n, np.uint32)
            self.image = adl.Buffer(dev, n, adl.float4)
        except Exception:
            self.release()
            raise
        self.frames_done = 0

    def params(self, frames: int, frame_begin: int) -> shim.AoParams:
        p = self.fill(shim.AoParams(), frames, frame_begin)
        p.num_triangles, p.rays_per_sample = self.num_triangles, self.rays_per_sample
        p.radius, p.miss_value = self.radius, self.miss_value
        return p

    def render(self, frames: int, frame_begin: Optional[int] = None, *, sync: Optional[adl.SyncObject] = None) -> None:
        """Enqueue frames [frame_begin, frame_begin + frames) (default: continue after the last call); frame_begin 0 starts the
        counts afresh.  The image is resolved from the counts afterwards."""
        frames, frame_begin = frame_range(frames, frame_begin, self.frames_done)
        if (frame_begin + frames) * self.rays_per_sample > 0xffffffff:
            raise ValueError("(frame_begin + frames) x rays_per_sample exceeds 2^32 - 1: the counts could wrap")
        p = self.params(frames, frame_begin)
        shim.check(self._lib.pt_render_ao(self.dev._h, self.tbuf._h, self.counts._h, self.image._h, ctypes.byref(p), self._cam_ref(),
                                          adl._handle(sync)))
        self.frames_done = frame_begin + frames

    def read_counts(self) -> np.ndarray:
        """uint32 [local_rows, width, 2]: {open, hits} per local pixel (synchronises)."""
        out = np.zeros((self.local_pixels, 2), np.uint32)
        if self.local_pixels:
            self.counts.read(out, 2 * self.local_pixels)
        self.dev.waitForCompletion()
        return out.reshape(self.local_rows, self.width, 2)

    def read_image(self) -> np.ndarray:
        """float32 [local_pixels, 4]: the AO image in the renderer's framebuffer layout, (a, a, a, 1) (synchronises)."""
        out = np.zeros((self.local_pixels, 4), np.float32)
        if self.local_pixels:
            self.image.read(out, self.local_pixels)
        self.dev.waitForCompletion()
        return out

    def read(self) -> np.ndarray:
        """float32 [local_rows, width]: the AO value per local pixel (synchronises)."""
        return self.read_image()[:, 0].reshape(self.local_rows, self.width)

    def release(self) -> None:
        for b in (self.counts, self.image):
            if b is not None:
                b.release()
        self.counts = self.image = None
        self.scene.release()


def resolve(counts: np.ndarray, rays_per_sample: int, miss_value: float = 1.0) -> np.ndarray:
    """The device's image rule on host counts {open, hits}: float32 open / (K hits) (each rounded to float, one division; K hits in
    uint32), miss_value where hits = 0."""
    c = np.asarray(counts, np.uint32)
    open_, hits = c[..., 0], c[..., 1]
    den = (np.uint32(rays_per_sample) * hits).astype(np.uint32)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = open_.astype(np.float32) / np.maximum(den, 1).astype(np.float32)
    return np.where(hits > 0, a, np.float32(miss_value)).astype(np.float32)
