"""Indirect illumination on the device (``pt_render_indirect``): the IndirectIllumination case the reference's harness declares --
the renderer's multi-bounce path with direct illumination's light sample taken at every vertex.

A sample of a pixel walks the renderer's path for up to ``max_bounces`` vertices.  At each vertex it takes ``light_samples`` (K)
points on the scene's emitters exactly as ``DirectRenderer`` does at the first, then the renderer's BRDF sample for the next ray.
The emitted light of a surface the path runs into counts at the first vertex only (later it is what the light samples of the
vertex before have gathered), so ``lights`` must hold every emissive triangle -- ``scene.emitters``, the default -- for an
unbiased image.  With an empty list the image is the renderer's at the same ``max_bounces``, with ``max_bounces=1`` it is
``DirectRenderer``'s, both bit for bit.  ``include/pt_shim.h`` states every step.  All compute is HIP in libptshim.so.
"""
from __future__ import annotations

from . import shim
from .direct import DirectRenderer
from .render import BOUNCES


class IndirectRenderer(DirectRenderer):
    """``DirectRenderer`` (its arguments, buffers, ``render`` / ``read`` / ``release``) with paths of up to ``max_bounces``
    vertices and ``light_samples`` light samples at each of them."""

    _PARAMS = shim.IndirectParams
    _ENTRY = "pt_render_indirect"

    def __init__(self, dev, triangles, materials, width: int, height: int, *, max_bounces: int = BOUNCES, **kw):
        self.max_bounces = int(max_bounces)
        if not 1 <= self.max_bounces <= 65535:
            raise ValueError("max_bounces must lie in 1..65535")
        super().__init__(dev, triangles, materials, width, height, **kw)

    def params(self, frames: int, frame_begin: int) -> shim.IndirectParams:
        p = super().params(frames, frame_begin)
        p.max_bounces = self.max_bounces
        return p
