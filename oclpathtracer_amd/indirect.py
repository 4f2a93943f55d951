"""Indirect illumination on the device (``pt_render_indirect``, ``pt_render_indirect_mis``): the IndirectIllumination case the
reference's harness declares -- the renderer's multi-bounce path with direct illumination's light sample taken at every vertex.

A sample of a pixel walks the renderer's path for up to ``max_bounces`` vertices.  At each vertex it takes ``light_samples`` (K)
points on the scene's emitters exactly as ``DirectRenderer`` does at the first, then the renderer's BRDF sample for the next ray.
The emitted light of a surface the path runs into counts at the first vertex only (later it is what the light samples of the
vertex before have gathered), so ``lights`` must hold every emissive triangle -- ``scene.emitters``, the default -- for an
unbiased image.  With an empty list the image is the renderer's at the same ``max_bounces``, with ``max_bounces=1`` it is
``DirectRenderer``'s, both bit for bit.

``mis=True`` renders with multiple importance sampling (the balance heuristic): a path that runs into an emitter at a later vertex
adds its light again, and that contribution and the light samples of the vertex before carry weights that sum to one.  The image
has the same expectation and, where glossy surfaces lie next to a light -- the Cornell box's own -- a third of the variance per
sample (DESIGN.md S4 has the measured ratios and rates).  The weights use the number of list entries per triangle, which the
renderer counts once on the device (``pt_light_counts``) into a buffer it owns; they make the image robust to a duplicated,
unsorted or incomplete list at every vertex but the path's last.  Both identities above hold with ``mis=True`` as well.

``light_choice="power"`` chooses the light of every light sample in proportion to its emitted power, as for ``DirectRenderer``
(``pt_render_indirect_power``; with ``mis=True`` the weights use the table's probabilities).  Both identities hold with it as well.

``roulette=Roulette(first_bounce=3, max_survival=0.95)`` -- or a bare int, the first bounce, with 0.95 -- ends paths early at random
(``pt_render_indirect_rr``): from vertex ``first_bounce`` on (counted from 1) a path survives its BRDF sample with probability
min(largest channel of its throughput, ``max_survival``) and is divided by that probability when it does, so the image's expectation
is unchanged while most of the searches a deep path spends on a throughput of a few percent are saved.  It composes with ``mis``,
``light_choice`` and ``moments``; ``None`` makes exactly the calls of a renderer without it.  A ``first_bounce`` of ``max_bounces`` or more
plays no roulette and gives the parent's image bit for bit.

``candidates=M`` (with ``light_choice="power"``) resamples every light sample of every vertex as ``DirectRenderer`` does
(``pt_render_indirect_ris``; without ``roulette`` none is played).  It composes with ``mis``, ``roulette``, ``moments`` and
``render_adaptive``, which then renders its lists through ``pt_render_indirect_pixels_ris``.

``environment=env, env_samples=Ke`` (with ``mis=True`` and ``light_choice="power"``) lights the scene by an octahedral sky map as
``DirectRenderer`` does, at every vertex (``pt_render_indirect_env``): a ray that leaves the scene adds the map's texel, Ke environment
samples per vertex find what is small and bright in the sky, and the two are balanced as the emitter samples and the BRDF ray are.
It composes with ``roulette`` and ``moments``; not with ``candidates`` or ``render_adaptive``.

``render_adaptive`` (with ``moments=True``) spends later frames only on the pixels that are still noisy: after a uniform start the
device lists the pixels whose own relative standard error lies above a tolerance (``pt_adaptive_select``), renders further frames of
the listed pixels only (``pt_render_indirect_pixels``), each from its own frame number, and counts them (``pt_sample_moments_pixels``)
until the list is empty.  Every pixel still holds exactly what a uniform render holds for it after as many frames as it has received.

``include/pt_shim.h`` states every step.  All compute is HIP in libptshim.so.
"""
from __future__ import annotations

import collections
import ctypes
import math

import numpy as np

from . import adl, shim
from .direct import DirectRenderer, light_counts
from .render import BOUNCES


class Roulette(collections.namedtuple("Roulette", "first_bounce max_survival")):
    """Russian roulette for ``IndirectRenderer``: played from vertex ``first_bounce`` >= 1 on, survival probability at most
    ``max_survival`` in (0, 1]."""

    __slots__ = ()

    def __new__(cls, first_bounce: int = 3, max_survival: float = 0.95):
        if isinstance(first_bounce, bool) or int(first_bounce) != first_bounce or int(first_bounce) < 1:
            raise ValueError("first_bounce must be an integer of at least 1")
        cap = float(max_survival)
        if math.isnan(cap) or not 0.0 < cap <= 1.0:
            raise ValueError("max_survival must lie in (0, 1]")
        return super().__new__(cls, min(int(first_bounce), 0x7fffffff), cap)

    @classmethod
    def of(cls, value):
        """None, a Roulette, or a bare int (the first bounce, with the default max_survival)"""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
            return cls(int(value))
        raise TypeError("roulette must be None, a Roulette or an int (the first bounce)")


# what render_adaptive returns: the list length of every pass, the samples the call has rendered (the uniform start included), and
# sample_counts() after it
AdaptiveResult = collections.namedtuple("AdaptiveResult", "passes samples counts")


class IndirectRenderer(DirectRenderer):
    """``DirectRenderer`` (its arguments, buffers, ``render`` / ``read`` / ``release``) with paths of up to ``max_bounces``
    vertices and ``light_samples`` light samples at each of them; ``mis``: with multiple importance sampling; ``roulette``: a
    ``Roulette`` (or its first bounce), paths end early at random without bias (None: every path walks on).  ``moments=True`` and its
    ``variance`` / ``noise`` / ``render_until`` are ``DirectRenderer``'s, under every estimator."""

    _PARAMS = shim.IndirectParams
    _ENTRY = "pt_render_indirect"

    def __init__(self, dev, triangles, materials, width: int, height: int, *, max_bounces: int = BOUNCES, mis: bool = False,
                 roulette=None, **kw):
        self.max_bounces = int(max_bounces)
        self.mis = bool(mis)
        self.roulette = Roulette.of(roulette)
        if kw.get("environment") is not None and not self.mis:
            raise ValueError("an environment needs mis=True: the sky is balanced against the BRDF ray")
        self._rr = None if self.roulette is None else shim.Roulette(*self.roulette)
        self.counts = None
        self.pixel_list = None      # the list of render_adaptive, allocated by its first call
        self._adaptive = False      # an adaptive pass has run since the last start at frame 0: the pixels share no frame number
        if not 1 <= self.max_bounces <= 65535:
            raise ValueError("max_bounces must lie in 1..65535")
        super().__init__(dev, triangles, materials, width, height, **kw)
        if self.mis:
            try:
                self.counts = light_counts(self._lib, dev, self._lights_h(), len(self.lights), self.num_triangles)
            except Exception:
                self.release()
                raise

    def params(self, frames: int, frame_begin: int) -> shim.IndirectParams:
        p = super().params(frames, frame_begin)
        p.max_bounces = self.max_bounces
        return p

    def _call(self, p, sync) -> int:
        scene3 = (self.dev._h, self.tbuf._h, self.mbuf._h, self._lights_h())
        if self._env is not None:
            env, env_cdf, block = self._env
            return self._lib.pt_render_indirect_env(*scene3, adl._handle(self.counts), adl._handle(self.cdf), adl._handle(self.tri_q), env._h, env_cdf._h,
                                                    self.samples._h, self.fb._h, ctypes.byref(p), ctypes.byref(self._rr or shim.NO_ROULETTE), ctypes.byref(block),
                                                    self._cam_ref(), adl._handle(sync))
        if self._ris is not None:
            return self._lib.pt_render_indirect_ris(*scene3, *self._estimator(), self.samples._h, self.fb._h, ctypes.byref(p),
                                                    ctypes.byref(self._rr or shim.NO_ROULETTE),
                                                    ctypes.byref(self._ris), self._cam_ref(), adl._handle(sync))
        if self._rr is not None:
            return self._lib.pt_render_indirect_rr(*scene3, *self._estimator(), self.samples._h, self.fb._h, ctypes.byref(p),
                                                   ctypes.byref(self._rr), self._cam_ref(), adl._handle(sync))
        if self.light_choice == "power":
            return self._lib.pt_render_indirect_power(*scene3, *self._estimator(), self.samples._h, self.fb._h, ctypes.byref(p),
                                                      self._cam_ref(), adl._handle(sync))
        if not self.mis:
            return super()._call(p, sync)
        return self._lib.pt_render_indirect_mis(*scene3, self.counts._h, self.samples._h, self.fb._h, ctypes.byref(p), self._cam_ref(),
                                                adl._handle(sync))

    def _estimator(self):
        """(mis, counts, cdf, tri_q) as the entry points with an estimator argument take them: a handle the estimator does not read is None"""
        return int(self.mis), adl._handle(self.counts), adl._handle(self.cdf), adl._handle(self.tri_q)

    def render(self, frames: int, frame_begin=None, sync=None) -> None:
        """``DirectRenderer.render``; after an adaptive pass only a start at frame 0 is accepted: the pixels no longer share a frame
        number that a uniform render could continue from."""
        if self._adaptive:
            if frame_begin is None or int(frame_begin) != 0:
                raise ValueError("after render_adaptive the pixels share no frame number: render from frame_begin=0")
            self._adaptive = False
        super().render(frames, frame_begin, sync)

    def _restart(self) -> None:
        super()._restart()
        self._adaptive = False

    def set_environment(self, environment, env_samples: int = 0) -> None:
        if environment is not None and not self.mis:
            raise ValueError("an environment needs mis=True: the sky is balanced against the BRDF ray")
        super().set_environment(environment, env_samples)

    def sample_counts(self) -> np.ndarray:
        """uint32 per local pixel: the samples the pixel has received since the last start at frame 0, finite or rejected (n +
        rejected of its moments); synchronises."""
        self._need_moments()
        rec = np.zeros(self.local_pixels, shim.MOMENTS_DTYPE)
        if self.local_pixels and self._moments_valid:
            self.mom.read(rec.view(np.uint8), rec.nbytes)
            self.dev.waitForCompletion()
        return rec["n"] + rec["rejected"]   # (uint32: wraps as the record's fields do)

    def render_adaptive(self, tolerance: float, *, max_samples: int, min_samples: int = 16, frames_per_pass=None,
                        floor: float = 1e-2) -> AdaptiveResult:
        """Render until every local pixel's own relative standard error lies at or below ``tolerance`` or the pixel has ``max_samples``
        samples.  If fewer than ``min_samples`` frames are done, they are rendered uniformly first (``render``).  Then, pass by pass:
        the device lists the pixels that have received fewer than ``max_samples`` samples and have fewer than ``min_samples`` finite
        ones or b > tolerance^2 * (c + floor^2) -- b the squared standard error of the pixel's mean, c its squared mean, summed over the
        channels as ``noise()`` sums them --, the host reads the list's length (ONE HOST WAIT PER PASS, as ``render_until`` has), and
        ``frames_per_pass`` (default ``chunk_frames``) further frames of the listed pixels are rendered and counted.  It ends with an
        empty list.  ``max_samples`` is tested on entry to a pass, so a pixel may end with up to ``max_samples + frames_per_pass - 1``
        samples.  ``floor`` keeps a black pixel from never stopping.

        Stopping on a variance estimated from the very samples that are averaged biases the image; the bias enters
        only through the number of samples a pixel stops at: the pixel's value is the uniform render's after that many frames, bit
        for bit.  Returns ``AdaptiveResult``.  Afterwards ``render`` accepts frame_begin 0 only; ``variance``, ``noise`` and
        ``sample_counts`` work as they are, and a further ``render_adaptive`` goes on from the pixels' own counts."""
        self._need_moments()
        if self._env is not None:
            raise ValueError("render_adaptive does not render under an environment")
        tolerance, floor = float(tolerance), float(floor)
        min_samples, max_samples = int(min_samples), int(max_samples)
        fpp = self.chunk_frames if frames_per_pass is None else int(frames_per_pass)
        if not tolerance >= 0.0 or not floor >= 0.0:
            raise ValueError("tolerance and floor must not be negative or NaN")
        if min_samples < 0 or max_samples < 1 or fpp < 1 or max_samples + fpp > 0x7fffffff or min_samples > 0x7fffffff:
            raise ValueError("min_samples >= 0, max_samples >= 1, frames_per_pass >= 1, and frame numbers must stay below 2^31")
        rendered = 0
        if not self._adaptive and self.frames_done < min_samples:
            rendered = (min_samples - self.frames_done) * self.local_pixels
            self.render(min_samples - self.frames_done)
        passes = []
        if not (self.local_pixels and self._moments_valid):
            return AdaptiveResult((), rendered, self.sample_counts())
        if self.pixel_list is None:
            self.pixel_list = adl.Buffer(self.dev, self._lib.pt_adaptive_list_bytes(self.local_pixels), np.uint8)
        rule = shim.AdaptiveRule(tolerance * tolerance, floor * floor, min_samples, max_samples)
        rr = self._rr or shim.NO_ROULETTE
        header = np.zeros(1, np.uint32)
        while True:
            shim.check(self._lib.pt_adaptive_select(self.dev._h, self.mom._h, self.local_pixels, ctypes.byref(rule), self.pixel_list._h, None))
            self.pixel_list.read(header, header.nbytes)
            self.dev.waitForCompletion()
            listed = int(header[0])
            if listed == 0:
                break
            passes.append(listed)
            self._adaptive = True
            hold = min(self.samples.getSize() // (3 * listed), 0x7fffffff // listed)   # frames of this list a call may render: all of them are counted
            done = 0
            while done < fpp:
                k = min(hold, fpp - done)
                head = (self.dev._h, self.tbuf._h, self.mbuf._h, self._lights_h(), *self._estimator(), self.samples._h, self.fb._h,
                        self.pixel_list._h, listed, ctypes.byref(self.params(k, done)), ctypes.byref(rr))
                if self._ris is not None:
                    shim.check(self._lib.pt_render_indirect_pixels_ris(*head, ctypes.byref(self._ris), self._cam_ref(), None))
                else:
                    shim.check(self._lib.pt_render_indirect_pixels(*head, self._cam_ref(), None))
                shim.check(self._lib.pt_sample_moments_pixels(self.dev._h, self.samples._h, self.mom._h, self.pixel_list._h, listed, k, None))
                done += k
            rendered += listed * fpp
        return AdaptiveResult(tuple(passes), rendered, self.sample_counts())

    def radiance_caster(self, *, workspace_bytes=None):
        """A ``radiance.RadianceCaster`` on this renderer's own scene, light list, counts and table -- one prepared scene, one LBVH --
        with its ``light_samples``, ``max_bounces``, ``mis``, ``light_choice`` and ``roulette``.  Radiance queries take neither
        resampling nor an environment.  Release the caster before the renderer."""
        from .radiance import RadianceCaster, _WORKSPACE_BYTES

        if self._ris is not None or self._env is not None:
            raise ValueError("radiance queries take neither resampling (candidates) nor an environment")
        return RadianceCaster(self.dev, self.tbuf, self.mbuf, light_samples=self.light_samples, max_bounces=self.max_bounces, mis=self.mis,
                              light_choice=self.light_choice, roulette=self.roulette,
                              workspace_bytes=_WORKSPACE_BYTES if workspace_bytes is None else workspace_bytes, _share=self)

    def release(self) -> None:
        for name in ("counts", "pixel_list"):
            if getattr(self, name) is not None:
                getattr(self, name).release()
                setattr(self, name, None)
        super().release()
