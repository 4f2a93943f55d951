"""The thin lens without a GPU: pt_camera's layout, pt_camera_derive's validation of the lens, and the geometry of the restatement's
lens ray (tests/lens_oracles.c, the expressions of include/pt_shim.h) -- the pinhole identity, the focus sphere, the disc, the circle of
confusion.  The GPU tests (tests/test_gpu_lens.py) hold the device to that restatement bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import direct_oracle as do
import indirect_oracle as io
import lens_oracle as lo
import lens_support as ls
from oclpathtracer_amd import scene, shim
from oclpathtracer_amd.camera import Camera

REF = ((0.0, 2.75, 4.0), (0.0, 2.75, 3.0), (0.0, 1.0, 0.0), 60.0)
NAN, INF = float("nan"), float("inf")


def _derive(R=0.0, F=0.0, reserved=None):
    c = shim.Camera()
    c.eye[:], c.center[:], c.up[:], c.fov_y_deg = REF
    c.lens_radius, c.focus_distance = R, F
    if reserved is not None:
        c.reserved[reserved] = 1
    out = np.full(16, -7.25, np.float32)
    rc = shim.load().pt_camera_derive(ctypes.byref(c), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return rc, out


def test_struct_layout():
    assert ctypes.sizeof(shim.Camera) == 64
    assert shim.Camera.lens_radius.offset == 40 and shim.Camera.focus_distance.offset == 44
    assert shim.Camera.reserved.offset == 40 and shim.Camera.reserved.size == 24
    c = shim.Camera()
    assert list(c.reserved) == [0] * 6 and c.lens_radius == 0.0 and c.focus_distance == 0.0
    c.lens_radius, c.focus_distance = 0.25, 6.0
    assert list(c.reserved) == [0x3e800000, 0x40c00000, 0, 0, 0, 0]   # the six-word view shows the floats' bits
    c.reserved[0] = 0x3f800000
    assert c.lens_radius == 1.0
    shim.load().pt_camera_reference(ctypes.byref(c))
    assert list(c.reserved) == [0] * 6   # the reference's camera has no lens


@pytest.mark.parametrize("R,F,reserved", [
    (-1.0, 4.0, None), (NAN, 4.0, None), (INF, 4.0, None), (-INF, 4.0, None),
    (0.0, -1.0, None), (0.1, -1.0, None), (0.0, NAN, None), (0.1, NAN, None), (0.0, INF, None), (0.1, INF, None),
    (0.1, 0.0, None), (0.1, -0.0, None), (1e-45, 0.0, None),
    (0.0, 0.0, 2), (0.0, 0.0, 3), (0.0, 0.0, 4), (0.0, 0.0, 5), (0.1, 6.0, 2), (0.1, 6.0, 5),
])
def test_invalid_lenses_are_rejected(R, F, reserved):
    rc, out = _derive(R, F, reserved)
    assert rc == shim.PT_ERR_INVALID
    assert np.all(out == np.float32(-7.25)), "a rejected camera wrote derived values"
    if reserved is None:
        with pytest.raises(ValueError):
            Camera(*REF, lens_radius=R, focus_distance=F)
        assert lo.lib().olens_set(R, F) == -1, "the restatement accepts a lens the library rejects"


@pytest.mark.parametrize("R,F", [(0.0, 0.0), (-0.0, 0.0), (-0.0, 5.0), (0.0, 5.0), (0.05, 6.0), (3.0, 0.5), (1e-45, 1e-45), (3e38, 3e38)])
def test_valid_lenses_and_their_derived_values(R, F):
    rc, out = _derive(R, F)
    assert rc == shim.PT_OK
    want = np.array([0.0, 2.75, 4.0, 0.0, 0.0, -1.0, 1.0, -0.0, 0.0, 0.0, 1.0, 0.0, float.fromhex("0x1.279a74p-1"), R, F, 0.0], np.float32)
    assert out.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    c = Camera(*REF, lens_radius=R, focus_distance=F)
    assert c.derive().view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert lo.lib().olens_set(R, F) == 0
    lo.lib().olens_set(0.0, 0.0)


def test_python_camera_lens():
    ref = Camera.reference()
    assert ref.lens_radius == 0.0 and ref.focus_distance == 0.0
    assert Camera.fit(scene.load_model()[0]).lens_radius == 0.0
    c = ref.with_lens(0.1, 6.0)
    assert (c.eye, c.center, c.up, c.fov_y_deg) == (ref.eye, ref.center, ref.up, ref.fov_y_deg)
    assert c.lens_radius == float(np.float32(0.1)) and c.focus_distance == 6.0   # rounded to binary32, as the other fields are
    s = c.to_struct()
    assert s.lens_radius == np.float32(0.1) and s.focus_distance == 6.0 and list(s.reserved)[2:] == [0] * 4
    on = ref.with_lens(0.1, focus_on=(3.0, 2.75, 0.0))
    assert on.focus_distance == 5.0                                               # |(3, 0, -4)|
    assert ref.with_lens(0.0) == ref and c.with_lens(0.0) == ref                  # the way back to the pinhole
    for bad in (dict(), dict(focus_distance=6.0, focus_on=(0.0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            ref.with_lens(0.1, **bad)
    with pytest.raises(ValueError):
        ref.with_lens(0.1, focus_on=ref.eye)                                      # a distance of 0
    o, w = ref.pinhole_ray()
    assert o.tolist() == [0.0, 2.75, 4.0] and np.allclose(w, [0.0, 0.0, -1.0], atol=1e-7)
    _, w = ref.pinhole_ray(1.0, 0.0, aspect=2.0)                                  # the top right corner of a 2 : 1 image
    t = math.tan(math.radians(30.0))
    assert np.allclose(w, np.array([2.0 * t, t, -1.0]) / math.sqrt(5.0 * t * t + 1.0), atol=1e-6)


def _ids(W, H, frames):
    gid = np.tile(np.arange(W * H, dtype=np.int32), frames)
    return gid, np.repeat(np.arange(frames, dtype=np.int32), W * H)


@pytest.mark.parametrize("F", [0.0, 4.0, 7.5])
@pytest.mark.parametrize("cam", [None, "oblique"])
def test_pinhole_identity_on_the_restatement(F, cam):
    """olens_set(0, F): every sample of a 16 x 16 x 4 direct and indirect render is camera_oracle's, bit for bit"""
    tris, mats = scene.load_model()
    cam = None if cam is None else Camera(**ls.OBLIQUE)
    gid, frame = _ids(16, 16, 4)
    want_d = do.decisions(tris, mats, 16, 16, gid, frame, 2, cam=cam)
    want_i = io.samples(tris, mats, 16, 16, gid, frame, 2, 4, cam=cam)
    with lo.lens(0.0, F):
        got_d = do.decisions(tris, mats, 16, 16, gid, frame, 2, cam=cam)
        got_i = io.samples(tris, mats, 16, 16, gid, frame, 2, 4, cam=cam)
    for g, w in zip(got_d + got_i, want_d + want_i):
        assert g.tobytes() == w.tobytes()
    assert do.lib is not lo.lib, "the lens block left its library behind"


def _basis(cam):
    d = cam.derive().astype(np.float64)
    return d[0:3], d[3:6], d[6:9], d[9:12]


def _pair(cam, W, H, frames):
    """(lens origin, lens direction, pinhole direction) of every sample, float64: the two share the jitter draws"""
    gid, frame = _ids(W, H, frames)
    o, d = lo.rays(cam, W, H, gid, frame)
    _, d0 = lo.rays(cam, W, H, gid, frame, R=0.0, F=0.0)
    return o.astype(np.float64), d.astype(np.float64), d0.astype(np.float64)


@pytest.mark.parametrize("name", ["reference", "oblique"])
def test_focus(name):
    """the lens ray of each sample passes within 1e-5 F of that sample's own pinhole eye + F dir"""
    R, F = 0.25, 6.0
    cam = ls.CAMERAS[name](R, F)
    eye = _basis(cam)[0]
    o, d, d0 = _pair(cam, 64, 64, 1)
    v = (eye + F * d0) - o
    along = (v * d).sum(1) / (d * d).sum(1)
    dist = np.linalg.norm(v - along[:, None] * d, axis=1)
    print("focus, %s: largest distance %.3e of %.3e" % (name, dist.max(), 1e-5 * F))
    assert dist.max() <= 1e-5 * F
    assert np.linalg.norm(o - eye, axis=1).max() > 0.9 * R, "the lens was not sampled: the test would pass for a pinhole"


def _disc_stats(off, hol, up, R):
    n = len(off)
    z_r2 = ((off * off).sum(1).mean() / (R * R) - 0.5) / (0.2887 / math.sqrt(n))
    z_h = (off @ hol).mean() / (0.5 * R / math.sqrt(n))
    z_u = (off @ up).mean() / (0.5 * R / math.sqrt(n))
    return z_r2, z_h, z_u


@pytest.mark.parametrize("W,H,frames,figures", [(64, 64, 1, (-0.75, 0.56, -1.2)), (16, 16, 16, (0.72, 0.26, -0.37))])
def test_disc(W, H, frames, figures):
    """org - eye lies in the plane of holDir and upDir within 1e-6 R, within R (1 + 1e-6) of the eye, uniform in area: the mean of
    |org - eye|^2 / R^2 within 4 standard errors of 1/2, both in-plane mean offsets within 4 standard errors of 0.  On the reference's
    camera, whose view axis is a coordinate axis: there eye + holDir lx + upDir ly is exact along it.  (The standard errors these inputs
    sit at on the RNG stream alone are `figures`.)"""
    R = 0.25
    cam = ls.reference_lens(R, 6.0)
    eye, view, hol, up = _basis(cam)
    off = _pair(cam, W, H, frames)[0] - eye
    assert np.abs(off @ view).max() <= 1e-6 * R
    assert np.linalg.norm(off, axis=1).max() <= R * (1.0 + 1e-6)
    z = _disc_stats(off, hol, up, R)
    print("disc %dx%dx%d: %.2f %.2f %.2f standard errors" % ((W, H, frames) + z))
    assert all(abs(v) <= 4.0 for v in z)
    assert all(abs(v - f) < 0.02 * max(1.0, abs(f)) + 0.01 for v, f in zip(z, figures)), "the draws are not the stream's third and fourth"


def test_disc_oblique():
    """The same disc on the oblique camera.  Its origins are binary32 sums of two additions at |eye| + R each: along the view axis they
    are off the plane by up to |view|_1 (ulp(max |eye| + R) + ulp(R)) <= sqrt(3) (4.8e-7 + 3e-8) = 8.8e-7 plus the basis' own
    non-orthogonality (a few 1e-7 R), which exceeds 1e-6 R = 2.5e-7: the plane is held to that bound of the number format instead."""
    R = 0.25
    cam = ls.oblique_lens(R, 6.0)
    eye, view, hol, up = _basis(cam)
    off = _pair(cam, 64, 64, 1)[0] - eye
    ulp = lambda x: float(np.spacing(np.float32(x)))
    bound = math.sqrt(3.0) * (ulp(np.abs(eye).max() + R) + ulp(R)) + 4e-7 * R
    print("disc, oblique: off the plane by %.3e at most, bound %.3e" % (np.abs(off @ view).max(), bound))
    assert np.abs(off @ view).max() <= bound
    assert np.linalg.norm(off, axis=1).max() <= R * (1.0 + 1e-6)
    assert all(abs(v) <= 4.0 for v in _disc_stats(off, hol, up, R))


@pytest.mark.parametrize("name", ["reference", "oblique"])
@pytest.mark.parametrize("depth", [0.5, 1.0, 2.0])
def test_circle_of_confusion(name, depth):
    """on a wall perpendicular to the view axis at depth D = depth x F, lens rays land within R |1 - D / (F cos(theta))| (1 + 1e-4) of the
    pinhole ray's landing point, cos(theta) = dir . view; the mean squared offset is half that radius squared, within 4 standard errors"""
    R, F = 0.25, 6.0
    D = depth * F
    cam = ls.CAMERAS[name](R, F)
    eye, view, _, _ = _basis(cam)
    o, d, d0 = _pair(cam, 64, 64, 1)
    t = (D - (o - eye) @ view) / (d @ view)
    cos = d0 @ view
    land, land0 = o + t[:, None] * d, eye + d0 * (D / cos)[:, None]
    radius = R * np.abs(1.0 - D / (F * cos))
    offset = np.linalg.norm(land - land0, axis=1)
    print("circle of confusion, %s, D = %g: largest offset / radius %.6f" % (name, D, (offset / radius).max()))
    assert np.all(offset <= radius * (1.0 + 1e-4))
    z = ((offset * offset / (radius * radius)).mean() - 0.5) / (0.2887 / math.sqrt(len(offset)))
    print("    mean squared offset: %.2f standard errors" % z)
    assert abs(z) <= 4.0
