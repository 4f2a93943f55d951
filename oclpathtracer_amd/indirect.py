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

``include/pt_shim.h`` states every step.  All compute is HIP in libptshim.so.
"""
from __future__ import annotations

import collections
import ctypes
import math

import numpy as np

from . import adl, shim
from .direct import DirectRenderer
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
        self._rr = None if self.roulette is None else shim.Roulette(self.roulette.first_bounce, self.roulette.max_survival)
        self.counts = None
        if not 1 <= self.max_bounces <= 65535:
            raise ValueError("max_bounces must lie in 1..65535")
        super().__init__(dev, triangles, materials, width, height, **kw)
        if self.mis:
            try:
                self.counts = adl.Buffer(dev, max(self.num_triangles, 1), np.int32)
                shim.check(self._lib.pt_light_counts(dev._h, self.lbuf._h if len(self.lights) else None, len(self.lights),
                                                     self.num_triangles, self.counts._h, None))
            except Exception:
                self.release()
                raise

    def params(self, frames: int, frame_begin: int) -> shim.IndirectParams:
        p = super().params(frames, frame_begin)
        p.max_bounces = self.max_bounces
        return p

    def _call(self, p, sync) -> int:
        if self._rr is not None:
            power = self.light_choice == "power"
            return self._lib.pt_render_indirect_rr(self.dev._h, self.tbuf._h, self.mbuf._h, self.lbuf._h if len(self.lights) else None,
                                                   int(self.mis), self.counts._h if self.mis else None,
                                                   self.cdf._h if power else None, self.tri_q._h if power else None,
                                                   self.samples._h, self.fb._h, ctypes.byref(p), ctypes.byref(self._rr),
                                                   ctypes.byref(self._cam) if self._cam is not None else None,
                                                   sync._h if sync is not None else None)
        if self.light_choice == "power":
            return self._lib.pt_render_indirect_power(self.dev._h, self.tbuf._h, self.mbuf._h, self.lbuf._h if len(self.lights) else None,
                                                      int(self.mis), self.counts._h if self.mis else None, self.cdf._h, self.tri_q._h,
                                                      self.samples._h, self.fb._h, ctypes.byref(p),
                                                      ctypes.byref(self._cam) if self._cam is not None else None,
                                                      sync._h if sync is not None else None)
        if not self.mis:
            return super()._call(p, sync)
        return self._lib.pt_render_indirect_mis(self.dev._h, self.tbuf._h, self.mbuf._h, self.lbuf._h if len(self.lights) else None,
                                                self.counts._h, self.samples._h, self.fb._h, ctypes.byref(p),
                                                ctypes.byref(self._cam) if self._cam is not None else None,
                                                sync._h if sync is not None else None)

    def release(self) -> None:
        if self.counts is not None:
            self.counts.release()
            self.counts = None
        super().release()
