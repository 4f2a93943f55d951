#!/usr/bin/env python
"""call_trace.py -- every library call the Python package makes for a fixed script, one line per call: the host-side counterpart of
tools/kernel_streams.py.  Two versions of the package issue the same calls exactly when their traces are the same text.

    python tools/call_trace.py [--package DIR] [--out FILE]

``--package DIR``: the directory that holds the ``oclpathtracer_amd`` to trace (default: this checkout); with PT_SHIM_LIB set, a copy
of another version's ``*.py`` runs against this checkout's library.  A recording proxy stands in ``shim._lib`` before anything is
constructed.  A line is ``name(arguments) = result``:

* a handle is ``h<k>``, numbered where the library hands it out; a freed handle's number is not used again;
* any other address (a tensor's memory, a stream, a mapped pointer) is ``p<k>``, numbered by first appearance;
* a block passed by reference is the hex of its bytes, a result pointer is ``out`` (and a handle it receives follows as ``-> h<k>``);
* the source of ``pt_buffer_write`` is ``sha1:<12 hex digits>`` of the bytes written, the destination of ``pt_buffer_read`` ``host``.

The script renders the packaged Cornell box at 16 x 16 through every class of the package, once as rank 1 of 2 with stripes of 4 rows
and once whole (``script``).  Without a device the trace ends at the first ``pt_device_create``, and so does the tool, with status 2.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "oclpathtracer_amd", "data", "cornellbox.bin")
W = H = 16


class Recorder:
    """Stands in for the ctypes library: calls go through, and each leaves one line in ``lines``."""

    def __init__(self, lib, signatures):
        self._lib, self._signatures = lib, signatures
        self.lines = []
        self._handles, self._addresses = {}, {}
        self._next_handle = 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "pt_last_error":
            return fn
        argtypes = self._signatures[name][1]

        def call(*args):
            shown = [self._show(name, i, t, a, args) for i, (t, a) in enumerate(zip(argtypes, args))]
            result = fn(*args)
            line = "%s(%s)" % (name, ", ".join(shown))
            if self._signatures[name][0] is ctypes.c_void_p:
                line += " = %s" % self._address(result)
            elif result is not None:
                line += " = %d" % result
            for t, a in zip(argtypes, args):   # a handle handed out through a result pointer
                if t == ctypes.POINTER(ctypes.c_void_p) and name != "pt_host_alloc" and a is not None and a._obj.value:
                    self._handles[a._obj.value] = "h%d" % self._next_handle
                    line += " -> h%d" % self._next_handle
                    self._next_handle += 1
            if name in ("pt_buffer_free", "pt_event_destroy", "pt_device_destroy"):
                self._handles.pop(_value(args[0]), None)
            self.lines.append(line)
            return result
        return call

    def _address(self, value) -> str:
        if not value:
            return "NULL"
        if value in self._handles:
            return self._handles[value]
        return self._addresses.setdefault(value, "p%d" % len(self._addresses))

    def _show(self, name, i, argtype, a, args) -> str:
        if argtype is ctypes.c_void_p:
            if name == "pt_buffer_write" and i == 1:
                return "sha1:" + hashlib.sha1(ctypes.string_at(_value(a), args[2])).hexdigest()[:12]
            if name == "pt_buffer_read" and i == 1:
                return "host"
            return self._address(_value(a))
        if argtype is ctypes.c_char_p:
            return repr(a)
        if isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer):
            if a is None:
                return "NULL"
            if issubclass(argtype._type_, ctypes.Structure) and hasattr(a, "_obj"):
                return bytes(a._obj).hex()
            return "out"
        return str(int(a))


def _value(a):
    return a.value if isinstance(a, ctypes.c_void_p) else a


def script(pt, dev, tris, mats, share: dict, tensors: bool) -> None:
    """every class of the package on one image share (``share``: Renderer's sharding keywords); ``tensors``: the torch forms too"""
    import numpy as np

    whole = not share
    eye = pt.camera.Camera((0.3, 2.5, 3.5), (0.0, 2.5, 0.0))
    sky = pt.environment.Environment.constant(0.5, size=4)
    r = pt.render.Renderer(dev, tris, mats, W, H, **share)
    r.render(2)
    r.set_camera(eye)
    r.render(2)
    r.read()
    r.global_rows()

    ao = r.ao_renderer(rays_per_sample=2)
    ao.render(2)
    ao.read()
    ao.release()
    for kw in ({}, dict(light_choice="power"), dict(light_choice="power", candidates=4),
               dict(light_choice="power", environment=sky, env_samples=2)):
        d = r.direct_renderer(**kw)
        d.render(2)
        d.read()
        d.release()
    sky.release()

    ind = r.indirect_renderer(mis=True, roulette=3, moments=True, chunk_frames=2, max_bounces=4)
    ind.render(3)
    ind.variance()
    ind.noise()
    f = r.feature_renderer(features=("albedo", "depth"))
    f.render(2)
    f.variance("depth")
    if tensors:
        f.variance("albedo", as_tensor=True)
    f.moments("albedo")
    f.release()
    if whole:   # the denoiser and the reprojection take whole images
        for kw in ({}, dict(spatial_below=2)):
            dn, feats = ind.denoiser(**kw)
            dn.denoise(ind.mom, feats)
            if tensors:
                dn.denoise(ind.mom, feats, as_tensor=True)
            dn.release()
            feats.release()
        acc = ind.temporal()
        acc.render(1)
        acc.move(None)
        acc.render(1)
        acc.mean()
        acc.history()
        acc.release()
    ind.render_adaptive(0.05, max_samples=ind.frames_done + 1, min_samples=2, frames_per_pass=1)   # one pass over the noisy pixels
    ind.sample_counts()

    rc = r.ray_caster()
    rays = rc.camera_rays(W, H, 0)
    rc.closest(rays)
    rc.occluded(rays)
    rc.occluded(rays, early_exit=True)
    rad = ind.radiance_caster()
    rad.radiance(rays, 2)
    rad.radiance(rays, 1, sample_begin=2, accumulate=True)
    if tensors:
        rays_t = rc.camera_rays(W, H, 0, eye, as_tensor=True)
        rc.closest(rays_t)
        rc.occluded(rays_t)
        rad.radiance(rays_t, 2)
        rad.radiance(rays_t, 1, sample_begin=2, accumulate=True)
    rad.release()
    rc.release()
    ind.release()
    r.release()

    # the same classes on scenes of their own: arrays in, every buffer theirs to free
    for own in (pt.ao.AORenderer(dev, tris, W, H, rays_per_sample=2, **share),
                pt.direct.DirectRenderer(dev, tris, mats, W, H, **share),
                pt.indirect.IndirectRenderer(dev, tris, mats, W, H, max_bounces=2, light_choice="power", **share),
                pt.features.FeatureRenderer(dev, tris, mats, W, H, features=("normal",), **share)):
        own.render(1)
        own.release()
    rc = pt.query.RayCaster(dev, tris)
    rc.closest(rays[:5])
    rc.release()
    rad = pt.radiance.RadianceCaster(dev, tris, mats, mis=True, light_choice="power", roulette=3)
    rad.radiance(np.ascontiguousarray(rays[:5]), 2)
    rad.release()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--package", default=ROOT, help="the directory that holds the oclpathtracer_amd to trace")
    ap.add_argument("--out", default=None, help="write the trace here instead of standard output")
    ap.add_argument("--no-tensors", action="store_true", help="leave the torch tensor forms out of the script")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    try:
        import torch  # noqa: F401  (before the library, so that both bind to the same HIP runtime)
    except ImportError:
        pass
    import importlib
    import types

    shim = importlib.import_module("oclpathtracer_amd.shim")
    rec = Recorder(shim.load(), shim.SIGNATURES)
    shim._lib = rec   # before anything is constructed: every object caches what shim.load() gives it
    pt = types.SimpleNamespace(**{m: importlib.import_module("oclpathtracer_amd." + m) for m in (
        "adl", "ao", "camera", "direct", "environment", "features", "indirect", "query", "radiance", "render", "scene")})
    status = 0
    try:
        tris, mats = pt.scene.load_model(SCENE)
        pt.adl.init(pt.adl.TYPE_HIP)
        dev = pt.adl.DeviceUtils.allocate(pt.adl.TYPE_HIP, pt.adl.Config(0))
        for share in (dict(n_ranks=2, rank=1, stripe_rows=4), {}):
            script(pt, dev, tris, mats, share, not args.no_tensors)
        pt.adl.DeviceUtils.deallocate(dev)
        pt.adl.quit(pt.adl.TYPE_HIP)
    except shim.ShimError as e:
        print("call_trace: stopped at %s" % e, file=sys.stderr)
        status = 2
    text = "".join(line + "\n" for line in rec.lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
