"""Direct illumination on the device (``pt_render_direct``): the DirectIllumination case the reference's harness declares, built
from the reference's own steps -- its RNG stream, camera, triangle test, BRDF expressions and gamma running mean.

A sample of a pixel traces the renderer's primary ray; a miss is the background.  On a hit the sample takes the emitted light of
the surface and ``light_samples`` (K) points on the scene's emitters: a light triangle chosen uniformly from the light list, a
point chosen uniformly on it, the BRDF value towards it, the geometry term, and a shadow ray that an any-hit search finds occluded
or open.  The result is the renderer's framebuffer -- with no lights it is the renderer's image at ``max_bounces=1`` bit for bit.
``light_choice="power"`` chooses the light triangle in proportion to the power it emits instead (``pt_render_direct_power``, through a
table built once on the device by ``pt_light_table``): the same expectation, and far less noise where the emitters differ in size
or brightness.
``candidates=M`` (with ``light_choice="power"``) resamples every light sample (``pt_render_direct_ris``): M candidates are drawn from the
table, one is kept in proportion to its unshadowed contribution at the shading point, and the one shadow ray goes to it -- the same
expectation, and far less noise where many emitters have similar power and most of them are far from, or face away from, the point.
``environment=env`` (an ``environment.Environment``, with ``light_choice="power"``) takes the light of a ray that leaves the scene from
an octahedral sky map instead of the constant 0.45, and ``env_samples=Ke`` samples that map Ke times per hit in proportion to what its
texels emit (``pt_render_direct_env``): a small bright source in the sky -- a sun -- is found by sampling, not by chance.
``moments=True`` keeps per-pixel noise estimates beside the image: after every call the first and second moments of the samples'
linear radiance are taken from the workspace on the device (``pt_sample_moments``), and ``variance()``, ``noise()`` and
``render_until()`` read them -- a variance map, an image-wide figure of 48 bytes, and a render that stops at a noise level.
``include/pt_shim.h`` states every expression.  All compute is HIP in libptshim.so; nothing here has a CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes
from typing import Optional

import numpy as np

from . import adl, scene, shim
from .camera import Camera
from .environment import Environment, check_env_samples
from .features import variance_map
from .image import ImageRenderer, ImageShare, frame_range

_WORKSPACE_BYTES = 64 << 20   # the default workspace holds as many whole frames as fit in this, at most 64

# what noise() returns: the mean over pixels and channels of the unbiased variance of one sample's linear radiance; the image's
# relative standard error sqrt(sum of the pixels' squared standard errors / sum of their squared means); the pixels with at least two
# finite samples (the only ones both figures count); the finite samples and the samples rejected for a NaN or an infinity, all pixels
Noise = collections.namedtuple("Noise", "variance_per_sample relative_error pixels samples rejected")


def light_table(lib, dev: adl.Device, tbuf, num_triangles: int, mbuf, num_materials: int, lights_h, num_lights: int):
    """(cdf, tri_q): the selection table of a light list, built once on the device (pt_light_table) into two new buffers"""
    cdf = adl.Buffer(dev, lib.pt_light_table_bytes(num_lights) // 8, np.uint64)
    tri_q = adl.Buffer(dev, max(num_triangles, 1), np.uint32)
    try:
        shim.check(lib.pt_light_table(dev._h, tbuf._h, num_triangles, mbuf._h, num_materials, lights_h, num_lights, cdf._h, tri_q._h, None))
    except Exception:
        cdf.release()
        tri_q.release()
        raise
    return cdf, tri_q


def light_counts(lib, dev: adl.Device, lights_h, num_lights: int, num_triangles: int):
    """the list entries per triangle, counted once on the device (pt_light_counts) into a new buffer"""
    counts = adl.Buffer(dev, max(num_triangles, 1), np.int32)
    try:
        shim.check(lib.pt_light_counts(dev._h, lights_h, num_lights, num_triangles, counts._h, None))
    except Exception:
        counts.release()
        raise
    return counts


class DirectRenderer(ImageRenderer, scene.SceneHolder):
    """Direct illumination of a ``width`` x ``height`` image of ``triangles`` with ``materials`` on ``dev``.

    ``triangles`` / ``materials``: ``scene.TRIANGLE_DTYPE`` / ``scene.MATERIAL_DTYPE`` arrays (uploaded to buffers of this
    renderer's), or ``adl.Buffer``s that already hold them -- a renderer's own (``Renderer.direct_renderer``), so that both share
    one prepared scene and one LBVH (``num_triangles`` / ``num_materials`` then say how many records count, and ``lights`` must
    be given).  ``lights``: the triangle indices light samples are drawn from (None: ``scene.emitters``); an empty list leaves the
    emitted light alone.  ``light_choice``: ``"uniform"`` -- every entry of the list with the same probability -- or ``"power"`` --
    in proportion to area x emission; the renderer then owns the selection table.  ``candidates``: 1 .. 32 candidates per light sample
    (resampled importance sampling; more than 1 needs ``light_choice="power"``; 1 makes exactly the calls of a renderer without it).  ``chunk_frames`` sizes the sample workspace: that many
    frames are traced by one launch and folded by the next.  ``stripe_rows`` / ``n_ranks`` / ``rank`` select the rows this device
    owns, as for ``Renderer``.  The search follows the device's options exactly as renders do.  ``moments``: keep per-pixel moments
    of the samples (``variance``, ``noise``, ``render_until``); the image is the same bit for bit, ``render`` issues its frames as calls
    of at most ``chunk_frames`` frames, each followed by ``pt_sample_moments``, and accepts ``frame_begin`` 0 or ``frames_done`` only.
    Adaptive sampling (``render_adaptive``) is ``IndirectRenderer``'s alone: for direct illumination use ``IndirectRenderer(max_bounces=1)``,
    whose image is this renderer's bit for bit."""

    def __init__(self, dev: adl.Device, triangles, materials, width: int, height: int, *, light_samples: int = 1, lights=None,
                 camera: Optional[Camera] = None, num_triangles: Optional[int] = None, num_materials: Optional[int] = None,
                 stripe_rows: int = 16, n_ranks: int = 1, rank: int = 0, chunk_frames: Optional[int] = None,
                 light_choice: str = "uniform", moments: bool = False, candidates: int = 1, environment: Optional[Environment] = None,
                 env_samples: int = 0):
        if light_choice not in ("uniform", "power"):
            raise ValueError('light_choice must be "uniform" or "power"')
        self.light_choice = light_choice
        self.environment, self.env_samples, self._env = None, 0, None
        self.set_candidates(candidates)
        self._check_environment(environment, env_samples)
        self.cdf = self.tri_q = None
        self.moments = bool(moments)
        self.mom = self.summary = self.noise_map = None
        self._moments_valid = False   # the moments buffer holds this image's sums (a call from frame 0 has reset it)
        self.dev = dev
        self._lib = shim.load()
        self.light_samples = int(light_samples)
        ImageShare.__init__(self, width, height, stripe_rows, n_ranks, rank)
        if not 1 <= self.light_samples <= 256:
            raise ValueError("light_samples must lie in 1..256")
        if chunk_frames is not None and int(chunk_frames) < 1:
            raise ValueError("chunk_frames must be at least 1")
        self._set_camera(camera)
        self.samples = self.fb = None
        self.scene = scene.SceneBuffers(dev, triangles, num_triangles, materials, num_materials, lights)
        n = max(self.local_pixels, 1)
        if chunk_frames is None:
            chunk_frames = max(1, min(64, _WORKSPACE_BYTES // (12 * n)))
        self.chunk_frames = int(chunk_frames)
        self.samples = adl.Buffer(dev, 3 * n * self.chunk_frames, np.float32)
        self.fb = adl.Buffer(dev, n, adl.float4)
        self.frames_done = 0
        try:
            if self.moments:
                self.mom = adl.Buffer(dev, n * ctypes.sizeof(shim.PixelMoments), np.uint8)
                self.summary = adl.Buffer(dev, self._lib.pt_moments_summary_bytes(n), np.uint8)
            if self.light_choice == "power":
                self._build_table()
            self.set_environment(environment, env_samples)
        except Exception:
            self.release()
            raise

    def _build_table(self) -> None:
        """the selection table of the list, built once on the device (pt_light_table) into buffers of this renderer's"""
        self.cdf, self.tri_q = light_table(self._lib, self.dev, self.tbuf, self.num_triangles, self.mbuf, self.num_materials,
                                           self._lights_h(), len(self.lights))

    def set_candidates(self, candidates: int, through_ris: bool = False) -> None:
        """``candidates`` (1 .. 32) per light sample from the next render on; more than 1 needs ``light_choice="power"``.  The image of
        another M is another image: start again at frame 0.  ``through_ris``: with ``light_choice="power"``, render through the RIS
        entry points even with 1 candidate -- the parent's image bit for bit by the RIS kernels, which is what a measurement of their
        cost compares (``tools/ris_rates.py``); otherwise 1 candidate makes exactly the calls of a renderer without resampling."""
        if isinstance(candidates, bool) or int(candidates) != candidates or not 1 <= int(candidates) <= 32:
            raise ValueError("candidates must be an integer in 1..32")
        if (int(candidates) > 1 or through_ris) and self.light_choice != "power":
            raise ValueError('candidates > 1 needs light_choice="power": the candidates are drawn from the light table')
        if (int(candidates) > 1 or through_ris) and self.environment is not None:
            raise ValueError("an environment renders without resampling: candidates must be 1")
        self.candidates = int(candidates)
        self._ris = shim.Ris(self.candidates) if self.candidates > 1 or through_ris else None

    def _check_environment(self, environment, env_samples) -> int:
        """what an environment asks of the renderer, refused before any device call; returns Ke"""
        ke = check_env_samples(env_samples)
        if environment is None:
            if ke:
                raise ValueError("env_samples needs an environment")
            return 0
        if not isinstance(environment, Environment):
            raise TypeError("environment must be an environment.Environment")
        if self.light_choice != "power":
            raise ValueError('an environment needs light_choice="power"')
        if self._ris is not None:
            raise ValueError("an environment renders without resampling: candidates must be 1")
        return ke

    def set_environment(self, environment: Optional[Environment], env_samples: int = 0) -> None:
        """Render under ``environment`` with ``env_samples`` environment samples per vertex from now on (None: the constant sky); the
        map and its table are made on this device on first use and stay the environment's own.  The image of another sky is another
        image: the next render starts again at frame 0."""
        ke = self._check_environment(environment, env_samples)
        self.environment, self.env_samples = environment, ke
        self._env = None
        if environment is not None:
            self._env = environment.buffers(self.dev) + (environment.block(ke),)
        self._restart()

    def _restart(self) -> None:
        """another camera or another sky is another image: the next render starts at frame 0, and so do the figures"""
        self.frames_done = 0
        self._moments_valid = False

    # what a renderer with the same buffers and another entry point changes (indirect.IndirectRenderer)
    _PARAMS = shim.DirectParams
    _ENTRY = "pt_render_direct"

    def params(self, frames: int, frame_begin: int):
        p = self.fill(self._PARAMS(), frames, frame_begin)
        p.num_triangles, p.num_materials, p.num_lights = self.num_triangles, self.num_materials, len(self.lights)
        p.light_samples = self.light_samples
        return p

    def render(self, frames: int, frame_begin: Optional[int] = None, sync: Optional[adl.SyncObject] = None) -> None:
        """Enqueue frames [frame_begin, frame_begin + frames) (default: continue after the last call); frame_begin 0 starts the
        running mean afresh.  With ``moments`` the frames go out as calls of at most ``chunk_frames`` frames, each followed by the
        moments of its samples, and frame_begin must be 0 or ``frames_done``: a frame rendered twice would be counted twice."""
        frames, frame_begin = frame_range(frames, frame_begin, self.frames_done, resumes=self.moments, who="with moments a render")
        if self.moments and frames > 0:
            first, end = frame_begin, frame_begin + frames
            while first < end:
                k = min(self.chunk_frames, end - first)
                shim.check(self._call(self.params(k, first), sync if first + k == end else None))
                if self.local_pixels:
                    shim.check(self._lib.pt_sample_moments(self.dev._h, self.samples._h, self.mom._h, self.local_pixels, k, int(first == 0), None))
                first += k
            self._moments_valid = True
        else:
            shim.check(self._call(self.params(frames, frame_begin), sync))
            if frame_begin == 0:
                self._moments_valid = False   # (no frames from 0: the image starts afresh, and so do the figures)
        self.frames_done = frame_begin + frames

    def _call(self, p, sync) -> int:
        """the entry point's return code (a renderer with another argument list overrides this)"""
        if self._env is not None:
            env, env_cdf, block = self._env
            return self._lib.pt_render_direct_env(self.dev._h, self.tbuf._h, self.mbuf._h, self._lights_h(), self.cdf._h, self.tri_q._h, env._h,
                                                  env_cdf._h, self.samples._h, self.fb._h, ctypes.byref(p), ctypes.byref(block),
                                                  self._cam_ref(), adl._handle(sync))
        if self._ris is not None:
            return self._lib.pt_render_direct_ris(self.dev._h, self.tbuf._h, self.mbuf._h, self._lights_h(), self.cdf._h, self.tri_q._h,
                                                  self.samples._h, self.fb._h, ctypes.byref(p), ctypes.byref(self._ris), self._cam_ref(),
                                                  adl._handle(sync))
        if self.light_choice == "power":
            return self._lib.pt_render_direct_power(self.dev._h, self.tbuf._h, self.mbuf._h, self._lights_h(), self.cdf._h, self.tri_q._h,
                                                    self.samples._h, self.fb._h, ctypes.byref(p), self._cam_ref(), adl._handle(sync))
        return getattr(self._lib, self._ENTRY)(self.dev._h, self.tbuf._h, self.mbuf._h, self._lights_h(), self.samples._h, self.fb._h,
                                               ctypes.byref(p), self._cam_ref(), adl._handle(sync))

    def read(self) -> np.ndarray:
        """Local framebuffer as (local_rows * width, 4) float32, the renderer's layout (synchronises)."""
        out = np.zeros((self.local_pixels, 4), np.float32)
        if self.local_pixels:
            self.fb.read(out, self.local_pixels)
        self.dev.waitForCompletion()
        return out

    def _need_moments(self) -> None:
        if not self.moments:
            raise RuntimeError("this renderer keeps no moments: construct it with moments=True")

    def variance(self):
        """The unbiased variance of one sample's linear radiance, per local pixel and channel, from every frame rendered since the
        last start at frame 0: ``(var float32 [local_pixels, 3], n uint32 [local_pixels])``, n the pixel's finite samples (a pixel
        with n < 2 has variance 0).  Resolved on the device (``pt_moments_resolve``); synchronises."""
        self._need_moments()
        var, n, self.noise_map = variance_map(self, self.mom, self._moments_valid, self.noise_map)
        return var, n

    def noise(self) -> Noise:
        """The image-wide noise figures (``Noise``) of the frames rendered since the last start at frame 0, reduced on the device and
        read back in 48 bytes; synchronises.  Without a pixel of two finite samples both figures are NaN."""
        self._need_moments()
        raw = np.zeros(ctypes.sizeof(shim.NoiseSummary), np.uint8)
        if self.local_pixels and self._moments_valid:
            shim.check(self._lib.pt_moments_resolve(self.dev._h, self.mom._h, self.local_pixels, None, self.summary._h, None))
            self.summary.read(raw, raw.nbytes)
            self.dev.waitForCompletion()
        s = shim.NoiseSummary.from_buffer(raw)
        with np.errstate(divide="ignore", invalid="ignore"):
            per_sample = float(np.float64(s.var_sum) / np.float64(3 * s.pixels))
            relative = float(np.sqrt(np.float64(s.se2_sum) / np.float64(s.mean2_sum)))
        return Noise(per_sample, relative, s.pixels, s.samples, s.rejected)

    def render_until(self, relative_error: float, max_frames: int, check_every: Optional[int] = None) -> int:
        """Render on from ``frames_done``, ``check_every`` frames at a time (default ``chunk_frames``), until ``noise().relative_error``
        lies below ``relative_error`` or ``max_frames`` frames are done; returns ``frames_done``.  Every check reads the 48 bytes of the
        summary back: ONE HOST WAIT PER CHECK, so a small ``check_every`` serialises the host with the device."""
        self._need_moments()
        step = self.chunk_frames if check_every is None else int(check_every)
        if step < 1:
            raise ValueError("check_every must be at least 1")
        while self.frames_done < int(max_frames):
            self.render(min(step, int(max_frames) - self.frames_done))
            if self.noise().relative_error < relative_error:
                break
        return self.frames_done

    def denoiser(self, **kw):
        """``(Denoiser, FeatureRenderer)`` for this renderer's image (``denoise.for_renderer``): the feature renderer keeps albedo,
        normal, depth and emission, shares this renderer's scene buffers and camera and has rendered ``frames_done`` frames;
        ``d.denoise(self.mom, f)`` filters the image (render both on by the same number of frames before the next call).  ``kw`` are
        ``Denoiser``'s parameters, among them ``spatial_below`` (``denoise.SPATIAL_BELOW`` filters one-sample pixels too; at the default
        0 they pass through unfiltered).  ValueError for ``n_ranks != 1`` -- a rank's stripes are not a whole image -- and without
        ``moments=True``.  Both objects are the caller's to release, before this renderer."""
        from .denoise import for_renderer

        return for_renderer(self, **kw)

    def temporal(self, **kw):
        """A ``temporal.TemporalAccumulator`` on this renderer: ``render(frames)`` as before, and ``move(camera)`` carries the moments
        across a camera move (``pt_reproject``) instead of starting again.  ``kw`` are ``Reprojector``'s parameters.  ValueError
        without ``moments=True``, for ``n_ranks != 1`` and with a lens.  The accumulator is the caller's to release, before this
        renderer."""
        from .temporal import TemporalAccumulator

        return TemporalAccumulator(self, **kw)

    def release(self) -> None:
        for b in (self.samples, self.fb, self.cdf, self.tri_q, self.mom, self.summary, self.noise_map):
            if b is not None:
                b.release()
        self.cdf = self.tri_q = self.mom = self.summary = self.noise_map = None
        self.samples = self.fb = None
        self.scene.release()
