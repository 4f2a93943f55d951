"""The look-at camera on the host (no GPU): the camera oracle against the oracle, pt_camera_derive against the contract
(DESIGN.md S3), rejected cameras, and the Python Camera."""
import ctypes

import numpy as np
import pytest

import camera_oracle
from conftest import assert_fb_equal


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _shim_derive(eye, center, up, fov, reserved=None):
    from oclpathtracer_amd import shim

    c = shim.Camera()
    c.eye[:], c.center[:], c.up[:] = eye, center, up
    c.fov_y_deg = fov
    if reserved is not None:
        c.reserved[:] = reserved
    out = np.zeros(16, np.float32)
    rc = shim.load().pt_camera_derive(ctypes.byref(c), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return rc, out


REF = ((0.0, 2.75, 4.0), (0.0, 2.75, 3.0), (0.0, 1.0, 0.0), 60.0)


@pytest.mark.parametrize("W,H,frames,depth,frame_begin", [
    (40, 24, 2, 16, 0),
    (40, 24, 2, 2, 5),
    (64, 64, 1, 16, 3),
    (64, 64, 2, 2, 0),
])
def test_camera_oracle_with_the_reference_camera_is_the_oracle(oracle, cornell, W, H, frames, depth, frame_begin):
    """Pins the copied ray generation and gamma fold: the reference camera through camera_oracle.c is ptoracle bit for bit."""
    from oclpathtracer_amd.camera import Camera

    tris, mats = cornell
    init = np.random.default_rng(W + frame_begin).uniform(0.0, 1.0, (W * H, 4)).astype(np.float32)
    want, wst = oracle.render(tris, mats, W, H, frames, frame_begin=frame_begin, max_bounces=depth, fb=init.copy(), want_stats=True)
    got, gst = camera_oracle.render(tris, mats, W, H, frames, Camera.reference(), frame_begin=frame_begin, max_bounces=depth,
                                    fb=init.copy(), want_stats=True)
    assert_fb_equal(got, want, "camera oracle, reference camera")
    assert gst == wst


def test_reference_camera_derives_to_the_kernel_constants():
    from oclpathtracer_amd import shim

    c = shim.Camera()
    shim.load().pt_camera_reference(ctypes.byref(c))
    assert tuple(c.eye) == REF[0] and tuple(c.center) == REF[1] and tuple(c.up) == REF[2] and c.fov_y_deg == 60.0
    assert list(c.reserved) == [0] * 6 and ctypes.sizeof(shim.Camera) == 64
    rc, out = _shim_derive(*REF)
    assert rc == shim.PT_OK
    want = np.array([0.0, 2.75, 4.0, 0.0, 0.0, -1.0, 1.0, -0.0, 0.0, 0.0, 1.0, 0.0, float.fromhex("0x1.279a74p-1"), 0, 0, 0],
                    np.float32)
    assert np.array_equal(_bits(out), _bits(want)), (out, want)   # signed zeros included
    assert _bits(out[12]) == _bits(np.float32(float.fromhex("0x1.279a74p-1")))


def test_derive_matches_the_camera_oracle_on_random_cameras():
    from oclpathtracer_amd import shim

    rng = np.random.default_rng(20261016)
    n_ok = 0
    for _ in range(300):
        eye = rng.uniform(-50, 50, 3).astype(np.float32)
        center = (eye + rng.normal(0, 1, 3) * rng.choice([1e-3, 1.0, 30.0])).astype(np.float32)
        up = rng.normal(0, 1, 3).astype(np.float32)
        fov = np.float32(rng.uniform(0.5, 179.5))
        rc, got = _shim_derive(eye, center, up, fov)
        want = camera_oracle.derive(eye, center, up, fov)
        assert (rc == shim.PT_OK) == (want is not None)
        if want is not None:
            n_ok += 1
            assert np.array_equal(_bits(got), _bits(want)), (eye, center, up, fov)
    assert n_ok >= 290


@pytest.mark.parametrize("eye,center,up,fov,reserved", [
    ((float("nan"), 2.75, 4.0), REF[1], REF[2], 60.0, None),
    (REF[0], (0.0, float("inf"), 3.0), REF[2], 60.0, None),
    (REF[0], REF[1], REF[2], float("nan"), None),
    (REF[0], REF[0], REF[2], 60.0, None),                    # center == eye
    (REF[0], (0.0, 3.75, 4.0), (0.0, 1.0, 0.0), 60.0, None),  # up parallel to the view direction
    (REF[0], (0.0, 1.75, 4.0), (0.0, 2.0, 0.0), 60.0, None),  # ... antiparallel
    (REF[0], REF[1], (0.0, 0.0, 0.0), 60.0, None),           # no up
    (REF[0], REF[1], REF[2], 0.0, None),
    (REF[0], REF[1], REF[2], 180.0, None),
    (REF[0], REF[1], REF[2], -5.0, None),
    (REF[0], REF[1], REF[2], 60.0, [0, 0, 0, 1, 0, 0]),
])
def test_invalid_cameras_are_rejected(eye, center, up, fov, reserved):
    from oclpathtracer_amd import shim

    rc, _ = _shim_derive(eye, center, up, fov, reserved)
    assert rc == shim.PT_ERR_INVALID
    if reserved is None:
        assert camera_oracle.derive(eye, center, up, fov) is None


def test_python_camera_validates():
    from oclpathtracer_amd.camera import Camera

    ref = Camera.reference()
    assert ref == Camera((0, 2.75, 4), (0, 2.75, 3))
    assert np.array_equal(_bits(ref.derive()), _bits(_shim_derive(*REF)[1]))
    for bad in (dict(eye=(0, 0, 0), center=(0, 0, 0)), dict(eye=(0, 0, 0), center=(0, 1, 0)),
                dict(eye=(0, 0, 0), center=(0, 0, -1), fov_y_deg=180.0), dict(eye=(0, 0, 0), center=(0, 0, -1), fov_y_deg=0.0),
                dict(eye=(0, float("nan"), 0), center=(0, 0, -1)), dict(eye=(0, 0), center=(0, 0, -1))):
        with pytest.raises(ValueError):
            Camera(**bad)
    with pytest.raises(Exception):
        ref.eye = (1.0, 2.0, 3.0)   # frozen


def _inside_image(cam, tris, aspect=1.0):
    d = cam.derive().astype(np.float64)
    eye, view, hol, up, angle = d[0:3], d[3:6], d[6:9], d[9:12], d[12]
    pts = np.concatenate([np.asarray(tris[f])[:, :3] for f in ("p1", "p2", "p3")]).astype(np.float64) - eye
    z = pts @ view
    assert np.all(z > 0)
    x = np.abs(pts @ hol) / z
    y = np.abs(pts @ up) / z
    return bool(np.all(x <= angle * aspect) and np.all(y <= angle))


@pytest.mark.parametrize("view_dir,up,fov", [((0, 0, -1), (0, 1, 0), 60.0), ((1, -0.5, -1), (0, 1, 0), 40.0), ((0, -1, 0), (0, 0, -1), 90.0)])
def test_fit_frames_the_whole_scene(cornell, view_dir, up, fov):
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.camera import Camera

    soup, _ = scene.make_soup(2000)
    for tris in (cornell[0], soup):
        cam = Camera.fit(tris, view_dir=view_dir, up=up, fov_y_deg=fov)
        assert _inside_image(cam, tris)
        wide = Camera.fit(tris, view_dir=view_dir, up=up, fov_y_deg=fov, aspect=0.5)
        assert _inside_image(wide, tris, aspect=0.5)
