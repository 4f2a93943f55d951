"""Host drivers of the hot path.

* ``raycast_reference_loop`` -- the reference harness's frame loop, call for call
  (test/RaytraceTest.cpp:202-291 ``TEST_F(DeviceTest, RayCast)``), through the Adl-shaped API.
* ``Renderer``               -- the fused entry point ``pt_render_frames`` (one call = many frames)
  with image-stripe sharding parameters for multi-GPU.

All compute happens in libptshim.so on the GPU; nothing here has a CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import adl, image, scene, shim
from .camera import Camera

BOUNCES = 16        # GenerateColors.cl:5
NUM_TRIANGLES = 36  # GenerateColors.cl:6


def upload_scene(dev: adl.Device, triangles: np.ndarray, materials: np.ndarray):
    """Scene upload exactly as RaytraceTest.cpp:222-246 does it: map, element-wise copy, unmap.

    (The reference over-allocates both buffers 64x by passing bytes as the element count,
    :222-223; that quirk is not reproduced.)"""
    tbuf = adl.Buffer(dev, len(triangles), scene.TRIANGLE_DTYPE)
    mbuf = adl.Buffer(dev, len(materials), scene.MATERIAL_DTYPE)
    tb = tbuf.getHostPtr()
    mb = mbuf.getHostPtr()
    adl.DeviceUtils.waitForCompletion(dev)
    tb[:] = triangles
    mb[:] = materials
    tbuf.returnHostPtr(tb)
    mbuf.returnHostPtr(mb)
    adl.DeviceUtils.waitForCompletion(dev)
    return tbuf, mbuf


def raycast_reference_loop(dev: adl.Device, triangles: np.ndarray, materials: np.ndarray, dimension: int = 512,
                           frames: int = 10000, kernel_path: str = "../test/ClKernels/GenerateColors") -> np.ndarray:
    """RaytraceTest.cpp:216-290 with ``dimension`` and the frame count as parameters.

    Returns the framebuffer as an (H*W, 4) float32 array (what the reference maps at :272)."""
    frameBuff = adl.Buffer(dev, dimension * dimension, adl.float4)
    tBuffer, materialBuffer = upload_scene(dev, triangles, materials)
    frameCount = 0
    while frameCount != frames:
        res = np.array([dimension, dimension, frameCount, 0], np.int32)
        frameCount += 1
        bInfo = [adl.BufferInfo(tBuffer), adl.BufferInfo(materialBuffer), adl.BufferInfo(frameBuff)]
        launcher = adl.Launcher(dev, dev.getKernel(kernel_path, "GenerateColors"))
        launcher.setBuffers(bInfo, len(bInfo))
        launcher.setConst(res)
        launcher.launch1D(dimension * dimension)
        adl.DeviceUtils.waitForCompletion(dev)
    h = frameBuff.getHostPtr()
    adl.DeviceUtils.waitForCompletion(dev)
    out = np.array(h, copy=True)
    for b in (frameBuff, tBuffer, materialBuffer):
        b.release()
    return out


def refuse_lens(camera: Optional[Camera]) -> None:
    """The fused renderer (``Renderer`` and what is built on it: ``ProgressiveRenderer``, ``StripeImage``) takes no thin lens, as
    pt_render_frames_camera takes none: its kernels' primary-ray masks are built on origin == eye.  Raised before anything is enqueued."""
    if isinstance(camera, Camera) and camera.lens_radius > 0.0:
        raise ValueError("the fused renderer takes no thin lens (lens_radius > 0): use IndirectRenderer with no lights, which "
                         "renders the same image and takes the lens, or Camera.with_lens(0.0) for the pinhole")


class Renderer(image.ImageRenderer):
    """One device's share of an image, rendered with the fused multi-frame entry point.

    ``n_ranks``/``rank``/``stripe_rows`` select the rows this device owns (rows are
    dealt in stripes, round-robin); the local framebuffer holds exactly those rows.  With the
    defaults it is the whole image.  ``fb_device_ptr`` lets the framebuffer live in caller-owned
    device memory (a torch tensor) so a collective can move it without a copy.  ``camera`` (a :class:`Camera`; None =
    the reference's camera, through ``pt_render_frames`` exactly as before) is the viewpoint (``set_camera``).
    """

    def __init__(self, dev: adl.Device, triangles: np.ndarray, materials: np.ndarray, width: int, height: int, *,
                 n_ranks: int = 1, rank: int = 0, stripe_rows: int = 16, fb_device_ptr: Optional[int] = None,
                 want_stats: bool = False, camera: Optional[Camera] = None):
        self.dev = dev
        self._set_camera(camera)
        image.ImageShare.__init__(self, width, height, stripe_rows, n_ranks, rank, sized=False)   # (pt_render_frames refuses a bad size)
        self.num_triangles, self.num_materials = len(triangles), len(materials)
        self.tbuf, self.mbuf = upload_scene(dev, triangles, materials)
        self.fb = adl.Buffer(dtype=adl.float4)
        if fb_device_ptr is None:
            self.fb.allocate(dev, max(self.local_pixels, 1))
        else:
            self.fb.setRawPtr(dev, fb_device_ptr, max(self.local_pixels, 1))
        self.stats = None
        if want_stats:
            self.stats = adl.Buffer(dev, shim.PT_STAT_WORDS, np.uint64)
            self.stats.write(np.zeros(shim.PT_STAT_WORDS, np.uint64), shim.PT_STAT_WORDS)
        self.frames_done = 0

    def render(self, frames: int, *, frame_begin: Optional[int] = None, max_bounces: int = BOUNCES,
               sync: Optional[adl.SyncObject] = None, fb: Optional[adl.Buffer] = None) -> None:
        """Enqueue frames [frame_begin, frame_begin+frames) (default: continue after the last call).
        ``fb``: another framebuffer of the same size to render into (a pipeline's second buffer)."""
        if frame_begin is None:
            frame_begin = self.frames_done
        p = self.fill(shim.RenderParams(), int(frames), int(frame_begin))
        p.max_bounces = int(max_bounces)
        p.num_triangles, p.num_materials = self.num_triangles, self.num_materials
        if self._cam is None:
            shim.check(shim.load().pt_render_frames(self.dev._h, self.tbuf._h, self.mbuf._h, (fb or self.fb)._h, ctypes.byref(p),
                                                    adl._handle(self.stats), adl._handle(sync)))
        else:
            shim.check(shim.load().pt_render_frames_camera(self.dev._h, self.tbuf._h, self.mbuf._h, (fb or self.fb)._h, ctypes.byref(p),
                                                           self._cam_ref(), adl._handle(self.stats), adl._handle(sync)))
        self.frames_done = frame_begin + frames

    def _set_camera(self, camera: Optional[Camera]) -> None:
        """(a moved camera invalidates the running mean, GenerateColors.cl:314-321: ``set_camera`` restarts the accumulation)"""
        refuse_lens(camera)
        super()._set_camera(camera)

    def read(self) -> np.ndarray:
        """Local framebuffer as (local_rows*W, 4) float32 (synchronises)."""
        out = np.empty((self.local_pixels, 4), np.float32)
        if self.local_pixels:
            self.fb.read(out, self.local_pixels)
        self.dev.waitForCompletion()
        return out

    def read_stats_raw(self) -> np.ndarray:
        """All PT_STAT_WORDS work counters (uint64), as accumulated since the buffer was last zeroed."""
        if self.stats is None:
            raise ValueError("renderer was created without want_stats")
        out = np.zeros(shim.PT_STAT_WORDS, np.uint64)
        self.stats.read(out, shim.PT_STAT_WORDS)
        self.dev.waitForCompletion()
        return out

    def read_stats(self) -> dict:
        out = self.read_stats_raw()
        return {"samples": int(out[shim.PT_STAT_SAMPLES]), "rays": int(out[shim.PT_STAT_RAYS])}

    def ray_caster(self):
        """A :class:`query.RayCaster` over this renderer's triangle buffer: queries and renders share the device's prepared scene
        and LBVH, so interleaving them prepares and builds nothing again.  Release it before the renderer."""
        from .query import RayCaster

        return RayCaster(self.dev, self.tbuf, num_triangles=self.num_triangles)

    def ao_renderer(self, **kw):
        """An :class:`ao.AORenderer` of this renderer's image over its triangle buffer (keyword arguments: AORenderer's; the
        image size, camera and sharding default to this renderer's): AO renders and renders share the device's prepared scene and
        LBVH.  Release it before the renderer."""
        from .ao import AORenderer

        width, height = image.like(self, kw)
        return AORenderer(self.dev, self.tbuf, width, height, num_triangles=kw.pop("num_triangles", self.num_triangles), **kw)

    def direct_renderer(self, **kw):
        """A :class:`direct.DirectRenderer` of this renderer's image over its triangle and material buffers (keyword arguments:
        DirectRenderer's, ``light_choice``, ``candidates``, ``environment`` / ``env_samples`` and ``moments`` among them; the image size, camera and sharding default to this renderer's): direct-illumination renders and renders
        share the device's prepared scene and LBVH.  Without ``lights`` the list is ``scene.emitters`` of the scene read back from
        the buffers (which waits for the device, once).  Release it before the renderer."""
        from .direct import DirectRenderer

        return self._lit_renderer(DirectRenderer, kw)

    def indirect_renderer(self, **kw):
        """An :class:`indirect.IndirectRenderer` over this renderer's buffers, as :meth:`direct_renderer` gives a DirectRenderer
        (keyword arguments: IndirectRenderer's, ``max_bounces``, ``mis``, ``light_choice``, ``candidates``, ``roulette``, ``environment`` / ``env_samples`` and ``moments`` among them)."""
        from .indirect import IndirectRenderer

        return self._lit_renderer(IndirectRenderer, kw)

    def feature_renderer(self, **kw):
        """A :class:`features.FeatureRenderer` of this renderer's image over its triangle and material buffers (keyword arguments:
        FeatureRenderer's, ``features`` and ``workspace_frames`` among them; the image size, camera and sharding default to this
        renderer's): first-hit albedo, normal, depth and emission with their variances, over the samples the lit renders take, through
        the device's prepared scene and LBVH.  Release it before the renderer."""
        from .features import FeatureRenderer

        return FeatureRenderer.on(self, **kw)

    def _lit_renderer(self, cls, kw):
        width, height = image.like(self, kw)
        if kw.get("lights") is None:
            tris = np.zeros(self.num_triangles, scene.TRIANGLE_DTYPE)
            mats = np.zeros(self.num_materials, scene.MATERIAL_DTYPE)
            if self.num_triangles:
                self.tbuf.read(tris, self.num_triangles)
            if self.num_materials:
                self.mbuf.read(mats, self.num_materials)
            self.dev.waitForCompletion()
            kw["lights"] = scene.emitters(tris, mats)
        return cls(self.dev, self.tbuf, self.mbuf, width, height, num_triangles=self.num_triangles, num_materials=self.num_materials, **kw)

    def release(self) -> None:
        for b in (self.tbuf, self.mbuf, self.fb, self.stats):
            if b is not None:
                b.release()
