"""Temporal reprojection on the device (``pt_reproject``): carry the lit renderers' moments across a camera move.

Each pixel of the new view re-projects its first hit -- the mean depth ``pt_render_features`` keeps -- into the previous view and,
where the same surface was seen there (a depth and a normal test on each of the four bilinear taps), takes that view's history over:
the weighted mean of the taps' radiance moments, for as many samples as the taps had, capped at ``max_history``.  The moments are
sums, so the new camera's samples are accumulated on top by ``pt_sample_moments`` as if nothing had happened; ``Denoiser`` filters the
result unchanged.  The scene is static: the motion comes from the two cameras and the depth alone.  View-dependent radiance (glossy
reflections) ghosts under reprojection; a small ``max_history`` is the remedy.
``include/pt_shim.h`` states every expression.  All compute is HIP in libptshim.so; nothing here has a CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import adl, shim
from .camera import Camera
from .features import FEATURES, FeatureRenderer
from .image import check_size

# the values the numpy prototype settled on (Cornell box, an 8-frame history under a shifted and a panned camera: at 48 x 48 the median
# relative MSE of history plus two new frames is 0.015 against 0.065 for the two frames alone; at 96 x 96 one of 67 pixels hidden from
# the old eye takes history under min_weight 0.6, six under 0.25; max_noise 0.5 -- a record worth fewer than two samples -- keeps the
# history's fireflies out: 0.6 % of its pixels; profiles/reproject/quality.txt)
DEFAULTS = dict(max_history=32, tol_z=0.05, cos_min=0.9, min_weight=0.6, max_noise=0.5)


def _pinhole(camera: Optional[Camera]) -> Optional[shim.Camera]:
    s = Camera.struct_of(camera)
    if s is not None and s.lens_radius > 0.0:
        raise ValueError("reprojection takes pinhole cameras: lens_radius must be 0")
    return s


class Reprojector:
    """``pt_reproject`` for ``width`` x ``height`` images on ``dev``: owns the scratch, sized once.  The parameters are
    ``pt_reproject_params``' and are refused here as the library refuses them."""

    def __init__(self, dev: adl.Device, width: int, height: int, *, max_history: int = 32, tol_z: float = 0.05, cos_min: float = 0.9,
                 min_weight: float = 0.6, max_noise: float = 0.5):
        self.dev = dev
        self._lib = shim.load()
        self.width, self.height = check_size(width, height)
        if isinstance(max_history, bool) or int(max_history) != max_history or not 0 <= int(max_history) <= 0x7fffffff:
            raise ValueError("max_history must be an integer in 0 .. 2^31 - 1")
        p = shim.ReprojectParams()
        p.width, p.height, p.max_history = self.width, self.height, int(max_history)
        p.tol_z, p.cos_min, p.min_weight, p.max_noise = tol_z, cos_min, min_weight, max_noise
        if not (float(p.tol_z) > 0.0 and math.isfinite(float(p.tol_z))):   # (as binary32 holds it)
            raise ValueError("tol_z must be finite and > 0 in binary32")
        if not 0.0 <= float(p.cos_min) <= 1.0:
            raise ValueError("cos_min must lie in [0, 1]")
        if not 0.0 <= float(p.min_weight) < 1.0:
            raise ValueError("min_weight must lie in [0, 1)")
        if not (float(p.max_noise) >= 0.0 and math.isfinite(float(p.max_noise))):
            raise ValueError("max_noise must be finite and >= 0")
        self.params = p
        self.pixels = self.width * self.height
        self.scratch = None
        self.scratch = adl.Buffer(dev, self._lib.pt_reproject_scratch_bytes(self.width, self.height), np.uint8)

    @staticmethod
    def _feature_handles(features):
        """(normal, depth) handles of a FeatureRenderer: the depth is required, the normal may be missing"""
        if not isinstance(features, FeatureRenderer):
            raise TypeError("features must be a features.FeatureRenderer")
        if "depth" not in features.mom:
            raise ValueError("reprojection needs the depth feature")
        if not features._valid:
            raise ValueError("a feature renderer has rendered nothing yet")
        return adl._handle(features.mom.get("normal")), features.mom["depth"]._h

    def reproject(self, prev_colour: adl.Buffer, prev_features: FeatureRenderer, cur_features: FeatureRenderer,
                  prev_camera: Optional[Camera], cur_camera: Optional[Camera], out: adl.Buffer, info: Optional[adl.Buffer] = None,
                  sync: Optional[adl.SyncObject] = None) -> None:
        """Enqueue the history ``prev_colour`` (``pt_pixel_moments[width * height]``, seen from ``prev_camera``) as ``cur_camera`` sees
        it into ``out``, and ``(fx, fy, weight, history length)`` per pixel into ``info`` (float4, optional); does not wait.  The
        normal test runs when both feature renderers keep normals."""
        for f in (prev_features, cur_features):
            if isinstance(f, FeatureRenderer) and ((f.width, f.height) != (self.width, self.height) or f.n_ranks != 1):
                raise ValueError("the features must be those of the whole %dx%d image" % (self.width, self.height))
        pn, pd = self._feature_handles(prev_features)
        cn, cd = self._feature_handles(cur_features)
        if pn is None or cn is None:
            pn = cn = None
        pc, cc = _pinhole(prev_camera), _pinhole(cur_camera)
        ref = lambda s: ctypes.byref(s) if s is not None else None
        shim.check(self._lib.pt_reproject(self.dev._h, prev_colour._h, pn, pd, cn, cd, self.scratch._h, out._h, adl._handle(info),
                                          ctypes.byref(self.params), ref(pc), ref(cc), adl._handle(sync)))

    def release(self) -> None:
        if self.scratch is not None:
            self.scratch.release()
        self.scratch = None


class TemporalAccumulator:
    """A lit renderer that keeps its history across camera moves (``DirectRenderer.temporal``, ``IndirectRenderer.temporal``).

    Holds the renderer, two ``FeatureRenderer``s of all four features on the renderer's scene buffers -- ``features`` is the current
    camera's, so ``Denoiser.denoise(r.mom, acc.features)`` works unchanged --, a history buffer and a ``Reprojector`` (``kw`` are its
    parameters).  ``render(frames)`` renders lit frames and feature frames by the same count.  ``move(camera)`` re-projects the
    moments into the new view and lets the renderer go on from its frame count under the new camera.  The renderer's gamma framebuffer
    then mixes views: it is the running mean over every frame since frame 0, whatever camera took it, and is NOT exposed here -- read
    the image from the moments (``mean()``) or from the denoiser.  ValueError without ``moments=True``, for ``n_ranks != 1`` and with
    a lens."""

    def __init__(self, renderer, *, feature_frames: int = 1, **kw):
        if not getattr(renderer, "moments", False):
            raise ValueError("the accumulator carries the renderer's moments: construct it with moments=True")
        if renderer.n_ranks != 1:
            raise ValueError("reprojection works on whole images: n_ranks must be 1 (a rank's stripes are not an image)")
        _pinhole(renderer.camera)
        if int(feature_frames) < 1:
            raise ValueError("feature_frames must be at least 1")
        self.renderer = r = renderer
        self.feature_frames = int(feature_frames)
        self.width, self.height = r.width, r.height
        self.pixels = r.width * r.height
        self.reprojector = self.features = self._previous = self.history_buf = self.info_buf = None
        self._moved = False
        try:
            self.reprojector = Reprojector(r.dev, r.width, r.height, **kw)
            self.features = FeatureRenderer.on(r, features=FEATURES)
            self._previous = FeatureRenderer.on(r, features=FEATURES)
            self.history_buf = adl.Buffer(r.dev, self.pixels * shim.MOMENTS_DTYPE.itemsize, np.uint8)
            self.info_buf = adl.Buffer(r.dev, self.pixels, adl.float4)
            if r.frames_done:
                self.features.render(r.frames_done, 0)
        except Exception:
            self.release()
            raise

    def render(self, frames: int) -> None:
        """Enqueue ``frames`` more lit frames and as many feature frames under the current camera."""
        self.renderer.render(frames)
        self.features.render(frames)

    def move(self, camera: Optional[Camera]) -> None:
        """Go on from ``camera`` (None: the reference's): the moments become the history as the new camera sees it, and the next
        ``render`` accumulates on top of it.  Enqueues a copy, ``feature_frames`` feature frames under the new camera and the
        reprojection; the host waits for nothing.  Before the first frame it only sets the camera."""
        r = self.renderer
        _pinhole(camera)
        old = r.camera
        if r.frames_done == 0 or not r._moments_valid:
            r.set_camera(camera)
            self.features.set_camera(camera)
            return
        self.history_buf.write(r.mom, self.pixels * shim.MOMENTS_DTYPE.itemsize)                      # 1: the history
        self.features, self._previous = self._previous, self.features                            # 2: the new view's features
        self.features._set_camera(camera)
        self.features.render(self.feature_frames, r.frames_done, restart=True)
        self.reprojector.reproject(self.history_buf, self._previous, self.features, old, camera, r.mom, self.info_buf)   # 3
        r._set_camera(camera)                                                                    # 4: frames_done and the moments stand
        self._moved = True

    def _records(self) -> np.ndarray:
        rec = np.zeros(self.pixels, shim.MOMENTS_DTYPE)
        r = self.renderer
        if r._moments_valid:
            r.mom.read(rec.view(np.uint8), rec.nbytes)
        r.dev.waitForCompletion()
        return rec

    def mean(self) -> np.ndarray:
        """float32 [height, width, 3]: the mean linear radiance, history and new samples together (synchronises)."""
        rec = self._records()
        n = rec["n"].astype(np.float64)[:, None]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            return np.where(n > 0, rec["sum"] / n, 0.0).astype(np.float32).reshape(self.height, self.width, 3)

    def info(self) -> np.ndarray:
        """float32 [height, width, 4] of the last move: where the pixel's first hit fell in the previous view (fx, fy), the sum of the
        surviving taps' bilinear weights and the history length taken over; zeros before the first move (synchronises)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        if self._moved:
            self.info_buf.read(out, self.pixels)
        self.renderer.dev.waitForCompletion()
        return out

    def history(self) -> np.ndarray:
        """uint32 [height, width]: the samples of history each pixel took over at the last move (synchronises)."""
        return self.info()[..., 3].astype(np.uint32)

    def release(self) -> None:
        for o in (self.features, self._previous, self.reprojector, self.history_buf, self.info_buf):
            if o is not None:
                o.release()
        self.features = self._previous = self.reprojector = self.history_buf = self.info_buf = None
