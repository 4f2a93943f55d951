"""The Python host layer, without a device: the moments record's two descriptions agree, and every renderer refuses a bad image share
and a bad frame range before anything reaches the device."""
import ctypes
import os

import numpy as np
import pytest

import moments_oracle
from test_query_cpu import _FakeDevice


def _layout(struct):
    return [(name, getattr(struct, name).offset, getattr(struct, name).size) for name, _ in struct._fields_]


def test_moments_records_agree_field_by_field():
    """shim.MOMENTS_DTYPE is what the package decodes pt_pixel_moments through, shim.NoiseSummary what it decodes pt_noise_summary
    through: each against the other description of the same record, and both against include/pt_shim.h's sizes"""
    from oclpathtracer_amd import features, shim

    dt = shim.MOMENTS_DTYPE
    assert features.MOMENTS_DTYPE is dt
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == _layout(shim.PixelMoments)
    assert _layout(shim.PixelMoments) == [("sum", 0, 24), ("sum2", 24, 24), ("n", 48, 4), ("rejected", 52, 4)]
    assert dt.itemsize == ctypes.sizeof(shim.PixelMoments) == 56 and dt == moments_oracle.MOMENTS_DTYPE
    sd = moments_oracle.SUMMARY_DTYPE
    assert [(n, sd.fields[n][1], sd.fields[n][0].itemsize) for n in sd.names] == _layout(shim.NoiseSummary)
    assert _layout(shim.NoiseSummary) == [("var_sum", 0, 8), ("se2_sum", 8, 8), ("mean2_sum", 16, 8), ("pixels", 24, 8), ("samples", 32, 8),
                                          ("rejected", 40, 8)]
    assert sd.itemsize == ctypes.sizeof(shim.NoiseSummary) == 48
    for name, kind in (("var_sum", "f"), ("pixels", "u")):   # (the float fields are doubles, the counts unsigned)
        assert sd.fields[name][0].kind == kind
    assert isinstance(shim.NoiseSummary(1.5).var_sum, float) and shim.NoiseSummary(pixels=2 ** 63).pixels == 2 ** 63


def _scene():
    from oclpathtracer_amd import scene

    return np.zeros(2, scene.TRIANGLE_DTYPE), np.zeros(1, scene.MATERIAL_DTYPE)


def _make(name, width, height, **share):
    """the class's constructor on a stand-in device, with everything but the image share valid"""
    from oclpathtracer_amd import ao, denoise, direct, features, indirect, render, temporal

    dev, (tris, mats) = _FakeDevice(), _scene()
    if name == "Renderer":
        return render.Renderer(dev, tris, mats, width, height, **share)
    if name == "AORenderer":
        return ao.AORenderer(dev, tris, width, height, **share)
    if name in ("Denoiser", "Reprojector"):
        assert not share
        return {"Denoiser": denoise.Denoiser, "Reprojector": temporal.Reprojector}[name](dev, width, height)
    cls = {"DirectRenderer": direct.DirectRenderer, "IndirectRenderer": indirect.IndirectRenderer, "FeatureRenderer": features.FeatureRenderer}[name]
    return cls(dev, tris, mats, width, height, **share)


def _bare(name):
    """an instance with five frames done and no device: what ``render`` looks at before it refuses a frame range"""
    from oclpathtracer_amd import ao, direct, features, indirect

    cls = {"AORenderer": ao.AORenderer, "DirectRenderer": direct.DirectRenderer, "IndirectRenderer": indirect.IndirectRenderer,
           "FeatureRenderer": features.FeatureRenderer}[name]
    r = cls.__new__(cls)
    r.dev, r._lib, r.frames_done = _FakeDevice(), None, 5
    r.rays_per_sample, r.moments, r._adaptive = 16, True, False   # (whichever of them the class reads)
    return r


CLASSES = ("Renderer", "AORenderer", "DirectRenderer", "IndirectRenderer", "FeatureRenderer", "Denoiser", "Reprojector")
# What each class answers, as it always has.  sizes: ValueError, or None where the constructor asks nothing of the size itself and
# goes on to the device (the fused renderer leaves it to pt_render_frames).  stripes: ValueError, or None where the class has no
# sharding.  frames: ValueError, or None where the class checks no frame range (Renderer.render) or renders no frames.  resume:
# ValueError where a render must start at frame 0 or at frames_done (the lit renderers: with moments), None where any start goes.
ANSWERS = {
    "Renderer":         dict(sizes=None,       stripes=ValueError, frames=None,       resume=None),
    "AORenderer":       dict(sizes=ValueError, stripes=ValueError, frames=ValueError, resume=None),
    "DirectRenderer":   dict(sizes=ValueError, stripes=ValueError, frames=ValueError, resume=ValueError),
    "IndirectRenderer": dict(sizes=ValueError, stripes=ValueError, frames=ValueError, resume=ValueError),
    "FeatureRenderer":  dict(sizes=ValueError, stripes=ValueError, frames=ValueError, resume=ValueError),
    "Denoiser":         dict(sizes=ValueError, stripes=None,       frames=None,       resume=None),
    "Reprojector":      dict(sizes=ValueError, stripes=None,       frames=None,       resume=None),
}
SIZES = ((0, 4), (4, 0), (65536, 32768))                       # no pixel; 2^31 pixels, one more than an int32 index reaches
STRIPES = (dict(stripe_rows=0), dict(n_ranks=2, rank=2))
FRAMES = ((-1, 0), (1, -1), (2, 0x7fffffff - 1))               # (frames, frame_begin): negative; a sum above 2^31 - 1


@pytest.mark.parametrize("name", CLASSES)
def test_bad_shares_and_frame_ranges_are_refused_before_the_device(name):
    from oclpathtracer_amd import shim

    if not os.path.exists(shim.LIB_PATH):
        pytest.skip("libptshim.so is not built: the classes load it, and pt_local_rows judges the stripes")
    want = ANSWERS[name]
    for width, height in SIZES:
        # (the stand-in device fails the test with an AssertionError when anything reaches it)
        with pytest.raises(want["sizes"] or AssertionError, match="invalid image size" if want["sizes"] else "must fail before"):
            _make(name, width, height)
    if want["stripes"]:
        for share in STRIPES:
            with pytest.raises(want["stripes"], match="invalid stripe geometry"):
                _make(name, 4, 4, **share)
    if want["frames"]:
        for frames, begin in FRAMES:
            with pytest.raises(want["frames"], match="invalid frame range"):
                _bare(name).render(frames, begin)
    if want["resume"]:
        with pytest.raises(want["resume"], match=r"starts at frame 0 or at frames_done \(5\), not at 3"):
            _bare(name).render(1, 3)
