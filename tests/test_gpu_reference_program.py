"""The device against what the reference kernel's own program wrote, bit for bit.

tests/golden/reference_program/ holds framebuffers, primary rays and closest hits computed by the reference's kernel file itself,
compiled for the host over PTSPEC built-ins (tests/golden/make_reference_golden.py; tests/test_reference_program_cpu.py keeps the
fixtures equal to a fresh run and to the oracle).  Nothing here reads the reference or the library compiled from it: only the
fixtures, and the scenes that tests/reference_cases.py generates for them.  Scenes of fewer than 36 triangles, which the reference
rendered padded with zero-area triangles, are rendered unpadded -- except through the GenerateColors launch, which is the
reference's 36-triangle kernel and takes the padded buffer as the reference did."""
import json
import os

import numpy as np
import pytest

import reference_cases as rc
from conftest import GOLDEN, assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import adl, scene as _scene

pytestmark = pytest.mark.gpu

REF_GOLDEN = os.path.join(GOLDEN, "reference_program")
NO_LIGHTS = np.zeros(0, np.int32)

# every form a 36-triangle scene's render through pt_render_frames can take
FORMS = [dict(QUAD_FILTER=q, PRIMARY_MASKS=p) for q in (0, 1) for p in (1, 0)] + \
        [dict(SECONDARY_MASKS=0), dict(SECONDARY_MASKS=1), dict(ACCEL=1), dict(ACCEL=2),
         dict(CHUNK_FRAMES=1, CHECKPOINT=1), dict(CHUNK_FRAMES=1, CHECKPOINT=0)]


def _fixture(name):
    return np.load(os.path.join(REF_GOLDEN, name + ".npy"))


def _pad36(tris):
    out = np.zeros(36, tris.dtype)
    out[: len(tris)] = tris
    return out


def _generate_colors_loop(device, tris, mats, W, H, frames):
    """the reference's host loop: one GenerateColors launch of W * H work-items per frame, cRes = (W, H, frame, 0)"""
    fb = adl.Buffer(device, W * H, adl.float4)
    tb = adl.Buffer(device, len(tris), _scene.TRIANGLE_DTYPE)
    mb = adl.Buffer(device, len(mats), _scene.MATERIAL_DTYPE)
    try:
        tb.write(tris, len(tris))
        mb.write(mats, len(mats))
        fb.write(np.zeros((W * H, 4), np.float32), W * H)
        for z in range(frames):
            launcher = adl.Launcher(device, device.getKernel("../test/ClKernels/GenerateColors", "GenerateColors"))
            launcher.setBuffers([adl.BufferInfo(tb), adl.BufferInfo(mb), adl.BufferInfo(fb)], 3)
            launcher.setConst(np.array([W, H, z, 0], np.int32))
            launcher.launch1D(W * H)
        out = np.zeros((W * H, 4), np.float32)
        fb.read(out, W * H)
        device.waitForCompletion()
        return out
    finally:
        for b in (fb, tb, mb):
            b.release()


def test_manifest_names_the_cases():
    with open(os.path.join(REF_GOLDEN, "manifest.json")) as f:
        man = json.load(f)
    assert [(m["name"], m["scene"], m["W"], m["H"], m["frames"]) for m in man["renders"]] == [tuple(g) for g in rc.GOLDEN_RENDERS]
    assert man["edge_classes"] == list(rc.EDGE_CLASSES)


@pytest.mark.parametrize("case", rc.GOLDEN_RENDERS, ids=[g[0] for g in rc.GOLDEN_RENDERS])
def test_framebuffers(device, case):
    from oclpathtracer_amd.indirect import IndirectRenderer

    name, scene_name, W, H, frames = case
    tris, mats = rc.scene(scene_name)
    want = _fixture(name)
    assert want.shape == (W * H, 3)
    for form in FORMS:
        with options(device, **form):
            got = render(device, tris, mats, W, H, frames)
        assert_fb_equal(got[:, :3], want, "%s, pt_render_frames with %s" % (name, form))
        assert np.all(got[:, 3] == 1.0)
    got = _generate_colors_loop(device, _pad36(tris), mats, W, H, frames)
    assert_fb_equal(got[:, :3], want, "%s, one GenerateColors launch per frame" % name)
    r = IndirectRenderer(device, tris, mats, W, H, light_samples=1, lights=NO_LIGHTS, max_bounces=16, stripe_rows=1,
                         chunk_frames=frames)
    try:
        r.render(frames)
        got = r.read()
    finally:
        r.release()
    assert_fb_equal(got[:, :3], want, "%s, IndirectRenderer with no lights at 16 bounces" % name)


def test_camera_rays(device, cornell):
    """pt_camera_rays hands out the vector the reference passes to getRay (include/pt_shim.h); the fixture holds generateRay's
    result, which has passed getRay: so the device's rays go through the oracle's getRay -- one more normalisation, pinned to the
    reference's by tests/test_reference_program_cpu.py -- before they are compared"""
    from oclpathtracer_amd.query import RayCaster
    from oracle import refprog

    W, H, frames = rc.GOLDEN_RAYS
    rcast = RayCaster(device, cornell[0])
    try:
        for frame in frames:
            want = _fixture("rays_%dx%d_f%d" % (W, H, frame))
            got = rcast.camera_rays(W, H, frame).view(np.float32).reshape(-1, 8)
            origin, direction = refprog.Side("oracle").get_ray(got[:, :3], got[:, 4:7])
            assert_fb_equal(origin, want[:, :3], "origins of frame %d" % frame)
            assert_fb_equal(direction, want[:, 3:], "directions of frame %d" % frame)
            assert np.all(got[:, 3] == np.float32(1e20))
    finally:
        rcast.release()


@pytest.mark.parametrize("accel", [1, 2])
def test_closest_hits(device, accel):
    """the edge rays -- aimed at vertices, edges and shared diagonals, grazing, starting on a triangle, meeting two coincident
    triangles, zero, NaN and infinite -- by brute force and through the LBVH: triangle, t, p and n (which do not depend on u, v)"""
    from oclpathtracer_amd.query import RayCaster

    rays, hits = _fixture("edge_rays"), _fixture("edge_hits")
    cls = rays[:, 6].astype(np.int32)
    assert len(rays) == len(hits) and len(rays) >= 900
    for c in range(len(rc.EDGE_CLASSES)):
        assert np.any((cls == c) & (hits[:, 0] >= 0)), "the fixture holds no hit of class " + rc.EDGE_CLASSES[c]
    for name in ("cornell", "coincident"):
        k = np.flatnonzero(rc.edge_scene_of(cls) == name)
        q = np.zeros((len(k), 8), np.float32)
        q[:, :3], q[:, 3], q[:, 4:7] = rays[k, :3], np.float32(1e20), rays[k, 3:6]
        rcast = RayCaster(device, rc.scene(name)[0])
        try:
            with options(device, ACCEL=accel):
                got = rcast.closest(q)
        finally:
            rcast.release()
        want_tri = hits[k, 0].astype(np.int32)
        what = "%s, accel %d" % (name, accel)
        assert np.array_equal(got["tri"], want_tri), "%s: triangles differ at %s" % (what, np.flatnonzero(got["tri"] != want_tri)[:8])
        h = want_tri >= 0
        assert_fb_equal(np.concatenate([got["t"][h, None], got["p"][h], got["n"][h]], axis=1), hits[k, 1:][h], what)
        assert np.all(got["t"][~h] == np.inf)
        if name == "coincident":
            assert h.sum() >= 40 and not np.any(want_tri == 35), "the second of two coincident triangles won"
