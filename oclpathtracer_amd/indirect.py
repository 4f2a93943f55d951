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

``include/pt_shim.h`` states every step.  All compute is HIP in libptshim.so.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import adl, shim
from .direct import DirectRenderer
from .render import BOUNCES


class IndirectRenderer(DirectRenderer):
    """``DirectRenderer`` (its arguments, buffers, ``render`` / ``read`` / ``release``) with paths of up to ``max_bounces``
    vertices and ``light_samples`` light samples at each of them; ``mis``: with multiple importance sampling.  ``moments=True`` and its
    ``variance`` / ``noise`` / ``render_until`` are ``DirectRenderer``'s, under every estimator."""

    _PARAMS = shim.IndirectParams
    _ENTRY = "pt_render_indirect"

    def __init__(self, dev, triangles, materials, width: int, height: int, *, max_bounces: int = BOUNCES, mis: bool = False, **kw):
        self.max_bounces = int(max_bounces)
        self.mis = bool(mis)
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
