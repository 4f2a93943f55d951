"""The denoiser on the device (``pt_denoise``): a feature-guided a-trous filter over the moments the library already keeps -- the
lit renderers' per-pixel moments of the radiance (``DirectRenderer(moments=True)``) and a ``FeatureRenderer``'s moments of albedo,
normal, depth and emission over the same jittered samples.

``levels`` passes of one 5 x 5 kernel whose taps lie ``1 << i`` pixels apart in pass i; a tap counts for less the further its depth,
albedo, emission, normal and -- measured against the pixel's own noise -- luminance lie from the centre's.  The result is the filtered
mean radiance (linear, not the gamma framebuffer) and, in the fourth channel, the variance the filter leaves in it.
A pixel that holds ONE sample has no variance of its own: the filter leaves it as it is -- a one-frame render whole, and after a camera
move the pixels that took no history.  ``spatial_below=SPATIAL_BELOW`` (``pt_denoise_spatial``) gives such pixels the pooled variance of
their guide-similar 7 x 7 neighbourhood before the levels run, so that they are filtered like their neighbours.
``include/pt_shim.h`` states every expression.  All compute is HIP in libptshim.so; nothing here has a CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import adl, shim
from .features import FEATURES, FeatureRenderer
from .image import check_size
from .query import into_tensor

# the starting values of the numpy prototype the filter was designed on (Cornell box, 48 x 48, 8 frames: the relative MSE falls to
# 0.025 of the unfiltered mean's; profiles/denoise/quality.txt)
DEFAULTS = dict(levels=5, sigma_l=4.0, sigma_z=1.0, sigma_a=0.01, sigma_e=0.01, eps_l=1e-6, eps_z=1e-4, normal_squarings=7)
# the recommended ``spatial_below``: exactly the pixels whose variance is unknown (n = 1).  On the same Cornell data one frame's median
# relative MSE after the filter falls from 0.128 to 0.023; values above 2 measured WORSE (two frames: mean 0.21 -> 0.73 at 4, because a
# firefly's own two-sample variance is what lets the levels blur it away; profiles/denoise_spatial/quality.txt)
SPATIAL_BELOW = 2


class Denoiser:
    """The filter for ``width`` x ``height`` images on ``dev``: owns the scratch and the output, sized once.  The parameters are
    ``pt_denoise_params``' and are refused here as the library refuses them.  ``spatial_below``: 0 (the default) calls ``pt_denoise``,
    which leaves one-sample pixels unfiltered; anything else calls ``pt_denoise_spatial`` with that ``below`` -- a pixel with
    ``1 <= n < spatial_below`` takes the pooled variance of its neighbourhood.  ``SPATIAL_BELOW`` (2) is the recommended value; values
    above 2 measured worse here."""

    def __init__(self, dev: adl.Device, width: int, height: int, *, levels: int = 5, sigma_l: float = 4.0, sigma_z: float = 1.0,
                 sigma_a: float = 0.01, sigma_e: float = 0.01, eps_l: float = 1e-6, eps_z: float = 1e-4, normal_squarings: int = 7,
                 spatial_below: int = 0):
        self.dev = dev
        self._lib = shim.load()
        self.width, self.height = check_size(width, height)
        if not 0 <= int(levels) <= 8 or not 0 <= int(normal_squarings) <= 8:
            raise ValueError("levels and normal_squarings must lie in 0..8")
        p = shim.DenoiseParams()
        p.width, p.height, p.levels, p.normal_squarings = self.width, self.height, int(levels), int(normal_squarings)
        p.sigma_l, p.sigma_z, p.sigma_a, p.sigma_e, p.eps_l, p.eps_z = sigma_l, sigma_z, sigma_a, sigma_e, eps_l, eps_z
        for name in ("sigma_l", "sigma_z", "sigma_a", "sigma_e", "eps_l", "eps_z"):
            v = float(getattr(p, name))   # (as binary32 holds it)
            if not (v > 0.0 and math.isfinite(v)):
                raise ValueError("%s must be finite and > 0 in binary32" % name)
        if isinstance(spatial_below, bool) or int(spatial_below) != spatial_below or not 0 <= int(spatial_below) <= 0x7fffffff:
            raise ValueError("spatial_below must be an integer in 0 .. 2^31 - 1")
        self.params = p
        self.spatial = None
        if int(spatial_below):
            self.spatial = shim.DenoiseSpatialParams()
            self.spatial.below = int(spatial_below)
        self.pixels = self.width * self.height
        self.scratch = self.out = self._sync = None
        self.scratch = adl.Buffer(dev, self._lib.pt_denoise_scratch_bytes(self.width, self.height), np.uint8)
        try:
            self.out = adl.Buffer(dev, self.pixels, adl.float4)
        except Exception:
            self.release()
            raise

    def _guides(self, features):
        """the four guide handles of pt_denoise, in FEATURES' order; a feature the renderer does not keep is left out"""
        if features is None:
            return [None] * len(FEATURES)
        if not isinstance(features, FeatureRenderer):
            raise TypeError("features must be a features.FeatureRenderer")
        if (features.width, features.height) != (self.width, self.height) or features.n_ranks != 1:
            raise ValueError("the features must be those of the whole %dx%d image" % (self.width, self.height))
        if not features._valid:
            raise ValueError("the feature renderer has rendered nothing yet")
        return [adl._handle(features.mom.get(f)) for f in FEATURES]

    def _enqueue(self, colour: adl.Buffer, features, out_h, ev) -> None:
        if self.spatial is None:
            shim.check(self._lib.pt_denoise(self.dev._h, colour._h, *self._guides(features), self.scratch._h, out_h, ctypes.byref(self.params), ev))
        else:
            shim.check(self._lib.pt_denoise_spatial(self.dev._h, colour._h, *self._guides(features), self.scratch._h, out_h,
                                                    ctypes.byref(self.params), ctypes.byref(self.spatial), ev))

    def denoise(self, colour: adl.Buffer, features=None, *, as_tensor: bool = False):
        """Filter the image whose moments ``colour`` holds (``pt_pixel_moments[width * height]``: a lit renderer's ``mom``), guided by
        whichever of the four features ``features`` (a ``FeatureRenderer`` of the same image, or None) keeps: float32 ``[height,
        width, 4]`` -- r, g, b of the filtered mean radiance and its variance; synchronises.  ``as_tensor``: a tensor on the device
        instead, ordered on torch's current stream, without a host wait for the filter."""
        if as_tensor:
            import torch

            out = torch.zeros((self.height, self.width, 4), dtype=torch.float32, device="cuda:%d" % self.dev.m_deviceIdx)
            self._sync = into_tensor(self.dev, out, self._sync, lambda out_h, ev: self._enqueue(colour, features, out_h, ev))
            return out
        self._enqueue(colour, features, self.out._h, None)
        res = np.zeros((self.height, self.width, 4), np.float32)
        self.out.read(res, self.pixels)
        self.dev.waitForCompletion()
        return res

    def release(self) -> None:
        for b in (self.scratch, self.out, self._sync):
            if b is not None:
                b.release()
        self.scratch = self.out = self._sync = None


def for_renderer(renderer, **kw):
    """``(Denoiser, FeatureRenderer)`` for a lit renderer that keeps moments (``DirectRenderer.denoiser``): the feature renderer
    keeps all four features, shares the renderer's scene buffers and camera and is brought to the renderer's frame count.  ``kw`` are
    ``Denoiser``'s, ``spatial_below`` among them."""
    if renderer.n_ranks != 1:
        raise ValueError("the denoiser filters whole images: n_ranks must be 1 (a rank's stripes are not an image)")
    if not renderer.moments:
        raise ValueError("the denoiser filters the renderer's moments: construct it with moments=True")
    d = Denoiser(renderer.dev, renderer.width, renderer.height, **kw)
    f = None
    try:
        f = FeatureRenderer.on(renderer, features=FEATURES)
        if renderer.frames_done:
            f.render(renderer.frames_done, 0)
    except Exception:
        d.release()
        if f is not None:
            f.release()
        raise
    return d, f
