"""Radiance queries: path-traced radiance along rays of the caller's (``pt_radiance_rays``).

The lit renderers start a sample at a pixel of an image through a camera; the ray queries take any ray and return geometry.  A
``RadianceCaster`` takes any ray and returns light: every sample of a ray is ``IndirectRenderer``'s sample with Russian roulette -- light
samples at every vertex, ``mis``, ``light_choice``, the roulette with lane refill, the LBVH -- from the ray's closest search on.  That is
what a light probe, a lightmap or vertex bake, an irradiance sensor, a panoramic, orthographic or fisheye camera, or per-ray radiance
for a model trained in torch need; ``panorama_rays`` makes the rays of a camera the library does not have.

* ``RadianceCaster.radiance(rays, samples)`` -- ``RadianceResult(mean, variance, n, rejected)`` per ray: the mean and the unbiased
  variance of one sample's linear radiance (float32 ``[N, 3]``), the finite samples and the rejected ones (uint32 ``[N]``).  The I/O
  forms are ``RayCaster``'s: numpy ``RAY_DTYPE`` or float32 ``[N, 8]`` in gives numpy out (synchronous); a device torch float32
  ``[N, 8]`` in gives device tensors out on the caster's GPU, ordered against torch's current stream by device-side waits.
* ``IndirectRenderer.radiance_caster()`` -- a caster on the renderer's own scene, light list, counts and table: one prepared scene,
  one LBVH.

A ray's ``tmax`` is not read: a radiance ray is unbounded, as every path segment is.  Sample ``s`` of ray ``r`` depends on
``first_ray + r`` and ``sample_begin + s`` alone, so a ray set may be split over calls (``first_ray``) and a ray's samples over calls
(``sample_begin``, ``accumulate=True``) without changing a bit.  ``include/pt_shim.h`` states every step.  All compute is HIP in
libptshim.so; nothing here has a CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes
from typing import Optional

import numpy as np

from . import adl, scene, shim
from .direct import light_counts, light_table
from .image import check_size
from .indirect import Roulette
from .query import RAY_DTYPE, DeviceIO, _is_tensor, check_numpy_rays, check_tensor_rays, make_rays  # noqa: F401  (RAY_DTYPE: the record of the rays, for callers)
from .render import BOUNCES

_WORKSPACE_BYTES = 64 << 20   # the default sample workspace: the samples of every ray that fit are walked by one launch
_ID_MAX = 0x7fffffff

RadianceResult = collections.namedtuple("RadianceResult", "mean variance n rejected")


def check_range(num_rays: int, samples: int, sample_begin: int = 0, first_ray: int = 0) -> None:
    """what ``radiance`` asks of its numbers, refused before any device call: ray ids and sample numbers stay below 2^31"""
    for name, v in (("samples", samples), ("sample_begin", sample_begin), ("first_ray", first_ray)):
        if isinstance(v, bool) or int(v) != v or int(v) < 0:
            raise ValueError("%s must be a non-negative integer" % name)
    if int(sample_begin) + int(samples) > _ID_MAX:
        raise ValueError("sample_begin + samples exceeds 2^31 - 1")
    if int(first_ray) + int(num_rays) > _ID_MAX:
        raise ValueError("first_ray + the number of rays exceeds 2^31 - 1")


def panorama_rays(eye, width: int, height: int) -> np.ndarray:
    """The rays of a latitude-longitude panorama seen from ``eye``: a ``RAY_DTYPE`` array of ``width * height`` rays, ray
    ``y * width + x`` through the centre of pixel (x, y).  Longitude runs over the columns from -pi to pi about the y axis (the
    image's centre column looks along -z, as the reference's camera does), latitude over the rows from straight up to straight down."""
    e = np.asarray(eye, np.float64).reshape(-1)
    width, height = check_size(width, height, "panorama")
    if e.shape != (3,) or not np.all(np.isfinite(e)):
        raise ValueError("eye must be three finite numbers")
    phi = (np.arange(width, dtype=np.float64) + 0.5) / width * (2.0 * np.pi) - np.pi
    theta = (np.arange(height, dtype=np.float64) + 0.5) / height * np.pi
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    d = np.stack([st * np.sin(phi)[None, :], np.broadcast_to(ct, (height, width)), -st * np.cos(phi)[None, :]], axis=-1)
    return make_rays(np.broadcast_to(e, (width * height, 3)), d.reshape(-1, 3))


class RadianceCaster(scene.SceneHolder):
    """Radiance along rays through ``triangles`` with ``materials`` on ``dev``.

    ``triangles`` / ``materials`` / ``lights`` / ``num_triangles`` / ``num_materials``: as for ``DirectRenderer`` (arrays, or ``adl.Buffer``s
    that already hold them).  ``light_samples`` (K) light samples per vertex, paths of up to ``max_bounces`` vertices, ``mis`` and
    ``light_choice`` as for ``IndirectRenderer``; ``roulette``: a ``Roulette``, its first bounce, or None for none.  ``workspace_bytes``
    sizes the sample workspace, which holds whole samples of every ray (grown when one sample of a call's rays does not fit).  The
    search follows the device's options exactly as renders do."""

    def __init__(self, dev: adl.Device, triangles, materials, *, lights=None, light_samples: int = 1, max_bounces: int = BOUNCES,
                 mis: bool = False, light_choice: str = "uniform", roulette=None, workspace_bytes: int = _WORKSPACE_BYTES,
                 num_triangles: Optional[int] = None, num_materials: Optional[int] = None, _share=None):
        if light_choice not in ("uniform", "power"):
            raise ValueError('light_choice must be "uniform" or "power"')
        self.light_choice, self.mis = light_choice, bool(mis)
        self.light_samples, self.max_bounces = int(light_samples), int(max_bounces)
        self.roulette = Roulette.of(roulette)
        if not 1 <= self.light_samples <= 256:
            raise ValueError("light_samples must lie in 1..256")
        if not 1 <= self.max_bounces <= 65535:
            raise ValueError("max_bounces must lie in 1..65535")
        if isinstance(workspace_bytes, bool) or int(workspace_bytes) < 12:
            raise ValueError("workspace_bytes must hold at least one sample (12 bytes)")
        self._rr = shim.NO_ROULETTE if self.roulette is None else shim.Roulette(*self.roulette)
        self.dev = dev
        self._lib = shim.load()
        self.counts = self.cdf = self.tri_q = self.samples = None
        self._acc = None        # ("numpy" | "torch", N, the moments tensor or None): what accumulate=True continues
        self._shared = _share is not None   # a renderer's scene, list, counts and table: none of them is this caster's to free
        if self._shared:
            self.scene = _share.scene.borrowed()
            self.counts, self.cdf, self.tri_q = _share.counts, _share.cdf, _share.tri_q
        else:
            self.scene = scene.SceneBuffers(dev, triangles, num_triangles, materials, num_materials, lights)
        self._io = DeviceIO(dev)
        try:
            if not self._shared and self.mis:
                self.counts = light_counts(self._lib, dev, self._lights_h(), len(self.lights), self.num_triangles)
            if not self._shared and light_choice == "power":
                self.cdf, self.tri_q = light_table(self._lib, dev, self.tbuf, self.num_triangles, self.mbuf, self.num_materials,
                                                   self._lights_h(), len(self.lights))
            self.samples = adl.Buffer(dev, int(workspace_bytes), np.uint8)
        except Exception:
            self.release()
            raise

    def _workspace(self, n: int) -> adl.Buffer:
        """the sample workspace, grown to hold one sample of n rays"""
        if self.samples.getSize() < 12 * n:
            self.samples.release()
            self.samples = adl.Buffer(self.dev, 12 * n, np.uint8)
        return self.samples

    def _enqueue(self, rb, mb, nb, n: int, samples: int, sample_begin: int, first_ray: int, reset: bool, ev) -> None:
        """the radiance call into the moments mb, then their variance into the noise map nb (the event on the last of the two)"""
        p = shim.RadianceParams()
        p.num_rays, p.first_ray = n, first_ray
        p.sample_begin, p.sample_count = sample_begin, samples
        p.num_triangles, p.num_materials, p.num_lights = self.num_triangles, self.num_materials, len(self.lights)
        p.light_samples, p.max_bounces, p.reset = self.light_samples, self.max_bounces, int(reset)
        shim.check(self._lib.pt_radiance_rays(self.dev._h, self.tbuf._h, self.mbuf._h, self._lights_h(), int(self.mis),
                                              adl._handle(self.counts) if self.mis else None, adl._handle(self.cdf), adl._handle(self.tri_q), rb._h,
                                              self._workspace(n)._h, mb._h, ctypes.byref(p), ctypes.byref(self._rr), None))
        shim.check(self._lib.pt_moments_resolve(self.dev._h, mb._h, n, nb._h, None, ev))

    def radiance(self, rays, samples: int, *, sample_begin: int = 0, first_ray: int = 0, accumulate: bool = False) -> RadianceResult:
        """Samples ``[sample_begin, sample_begin + samples)`` of every ray; ray ``r`` has the id ``first_ray + r``.  ``accumulate``: go on
        from the moments of this caster's last call (the same number of rays, the same I/O form) instead of from zeros, so that calls
        over consecutive sample ranges equal one call bit for bit.  The mean is the ordered binary64 sum over the finite samples
        divided by their number, the variance ``pt_moments_resolve``'s, both rounded once to float32; a ray without a finite sample
        has mean 0, one with fewer than two variance 0."""
        if not isinstance(accumulate, bool):
            raise TypeError("accumulate must be a bool")
        tensor = _is_tensor(rays)
        if tensor:
            check_tensor_rays(rays, self.dev)
            n = int(rays.shape[0])
        else:
            r = check_numpy_rays(rays)
            n = len(r)
        check_range(n, samples, sample_begin, first_ray)
        samples, sample_begin, first_ray = int(samples), int(sample_begin), int(first_ray)
        form = "torch" if tensor else "numpy"
        go_on = accumulate and self._acc is not None
        if go_on and self._acc[:2] != (form, n):
            raise ValueError("accumulate=True continues the last call: %d %s rays, not %d %s rays" % (self._acc[1], self._acc[0], n, form))
        if tensor:
            return self._radiance_tensor(rays, n, samples, sample_begin, first_ray, go_on)
        mom = np.zeros(n, shim.MOMENTS_DTYPE)
        noise = np.zeros((n, 4), np.float32)
        if n:
            rb = self._io.staging("rays", r.nbytes)
            mb = self._io.staging("moments", mom.nbytes)
            nb = self._io.staging("noise", noise.nbytes)
            rb.write(r.view(np.uint8), r.nbytes)
            if not go_on:   # (a call of no samples enqueues nothing: the record starts from zeros here)
                mb.write(mom.view(np.uint8), mom.nbytes)
            self._enqueue(rb, mb, nb, n, samples, sample_begin, first_ray, not go_on, None)
            mb.read(mom.view(np.uint8), mom.nbytes)
            nb.read(noise.view(np.uint8).reshape(-1), noise.nbytes)
        self.dev.waitForCompletion()
        self._io.trim_wraps()
        self._acc = (form, n, None)
        cnt = mom["n"].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(cnt[:, None] > 0, mom["sum"] / cnt[:, None].astype(np.float64), 0.0).astype(np.float32)
        return RadianceResult(mean, np.ascontiguousarray(noise[:, :3]), cnt, mom["rejected"].copy())

    def _radiance_tensor(self, rays, n: int, samples: int, sample_begin: int, first_ray: int, go_on: bool) -> RadianceResult:
        import torch

        dev = rays.device
        mom = self._acc[2] if go_on else torch.zeros((n, shim.MOMENTS_DTYPE.itemsize // 8), dtype=torch.float64, device=dev)
        noise = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        if n:
            rays.record_stream(torch.cuda.current_stream(dev))
            self._io.on_tensors(lambda rb, mb, nb, ev: self._enqueue(rb, mb, nb, n, samples, sample_begin, first_ray, not go_on, ev),
                                rays, mom, noise)
        self._acc = ("torch", n, mom)
        # the record's fields as columns of its 32-bit words (torch has no structured dtype): n and rejected by their offsets
        words = mom.view(torch.int32).view(n, shim.MOMENTS_DTYPE.itemsize // 4)
        cnt, rej = (words[:, shim.MOMENTS_DTYPE.fields[f][1] // 4].contiguous() for f in ("n", "rejected"))
        cntd = (cnt.to(torch.int64) & 0xffffffff).to(torch.float64)[:, None]
        sums = mom[:, shim.MOMENTS_DTYPE.fields["sum"][1] // 8:][:, :3]
        mean = torch.where(cntd > 0, sums / cntd, torch.zeros_like(sums)).to(torch.float32)
        return RadianceResult(mean, noise[:, :3].contiguous(), cnt.view(torch.uint32), rej.view(torch.uint32))

    def release(self) -> None:
        self.scene.release()
        for b in (self.samples,) if self._shared else (self.counts, self.cdf, self.tri_q, self.samples):
            if b is not None:
                b.release()
        self._acc = None
        self._io.release()
        self.counts = self.cdf = self.tri_q = self.samples = None
