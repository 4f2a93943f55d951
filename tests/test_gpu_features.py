"""pt_render_features on the device, bit for bit against the CPU oracle (tests/feature_oracle.c; tests/test_features_cpu.py proves that
every input here reaches its edge): the four sample arrays compared as uint32 with NaN positions equal, through every search; the
oracle-free identity with pt_camera_rays + pt_intersect_rays; FeatureRenderer's moments, means and variances against the numpy
restatement of pt_sample_moments / pt_moments_resolve; the outputs left out, and the argument errors."""
import ctypes
import itertools

import numpy as np
import pytest

import feature_cases as fc
import feature_oracle as fo
import moments_oracle as mom
from conftest import assert_fb_equal
from gpu_support import SEARCHES, options
from oclpathtracer_amd import adl, scene, shim
from oclpathtracer_amd.camera import Camera

pytestmark = pytest.mark.gpu

E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
GUARD = np.float32(-7.25)


class Features:
    """The buffers of raw calls of pt_render_features on one case: the scene, and four outputs of ``frames`` frames, each with a guard
    word behind it and filled with the guard's value."""

    def __init__(self, device, name, W=fc.W, H=fc.H, frames=2, **stripes):
        self.device, self.lib = device, shim.load()
        self.tris, self.mats, self.cam = fc.case(name)
        self.W, self.H, self.frames, self.stripes = W, H, frames, stripes
        self.npix = fo.local_pixels(W, H, **stripes)
        self.tb = adl.Buffer(device, max(len(self.tris), 1), scene.TRIANGLE_DTYPE)
        self.mb = adl.Buffer(device, len(self.mats), scene.MATERIAL_DTYPE)
        if len(self.tris):
            self.tb.write(self.tris, len(self.tris))
        self.mb.write(self.mats, len(self.mats))
        self.words = 3 * self.npix * frames
        self.out = {f: adl.Buffer(device, self.words + 1, np.float32) for f in fo.FEATURES}
        self.fill()

    def fill(self):
        for b in self.out.values():
            b.write(np.full(self.words + 1, GUARD, np.float32), self.words + 1)

    def params(self, frames=None, frame_begin=0, **kw):
        p = shim.FeatureParams()
        p.width, p.height, p.frame_begin, p.frame_count = self.W, self.H, frame_begin, self.frames if frames is None else frames
        p.num_triangles, p.num_materials = len(self.tris), len(self.mats)
        p.stripe_rows, p.n_ranks, p.rank = (self.stripes.get(k, d) for k, d in (("stripe_rows", 1), ("n_ranks", 1), ("rank", 0)))
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    def call(self, p, which=fo.FEATURES, cam="case", **over):
        """the entry point on these buffers -- of the outputs only those ``which`` names, each buffer replaced by what ``over`` names for
        it (None: a NULL handle)"""
        bufs = {"tb": self.tb, "mb": self.mb}
        bufs.update({f: self.out[f] if f in which else None for f in fo.FEATURES})
        bufs.update(over)
        struct = Camera.struct_of(self.cam) if isinstance(cam, str) else cam
        h = [bufs[k]._h if bufs[k] is not None else None for k in ("tb", "mb") + fo.FEATURES]
        return self.lib.pt_render_features(self.device._h, *h, ctypes.byref(p) if p is not None else None,
                                           ctypes.byref(struct) if struct is not None else None, None)

    def read(self, name, frames=None):
        """(the samples float32 [frames, npix, 3], everything behind them up to and including the guard word)"""
        raw = np.zeros(self.words + 1, np.float32)
        self.out[name].read(raw, self.words + 1)
        self.device.waitForCompletion()
        k = 3 * self.npix * (self.frames if frames is None else frames)
        return raw[:k].reshape(-1, self.npix, 3), raw[k:]

    def assert_untouched(self, names=fo.FEATURES):
        for f in names:
            got, rest = self.read(f, 0)
            assert np.all(rest == GUARD), "%s was touched" % f

    def release(self):
        for b in [self.tb, self.mb] + list(self.out.values()):
            b.release()


def _assert_samples(b, want, what, names=fo.FEATURES, frames=None):
    for f in names:
        got, rest = b.read(f, frames)
        assert_fb_equal(got, getattr(want, f) if not isinstance(want, dict) else want[f], "%s: %s" % (what, f))
        assert np.all(rest == GUARD), "%s: %s was written behind its samples" % (what, f)


def _render(device, name, W=fc.W, H=fc.H, frames=2, frame_begin=0, **stripes):
    """one all-four call of a case: {feature: samples}"""
    b = Features(device, name, W, H, frames, **stripes)
    try:
        assert b.call(b.params(frame_begin=frame_begin)) == shim.PT_OK, b.lib.pt_last_error()
        out = {}
        for f in fo.FEATURES:
            out[f], rest = b.read(f)
            assert np.all(rest == GUARD), "%s: %s was written behind its samples" % (name, f)
        return out
    finally:
        b.release()


def _assert_case(device, name, W=fc.W, H=fc.H, frames=2, **stripes):
    got = _render(device, name, W, H, frames, **stripes)
    want = fc.oracle(name, W, H, frames, **stripes)
    for f in fo.FEATURES:
        assert_fb_equal(got[f], getattr(want, f), "%s %dx%dx%d: %s" % (name, W, H, frames, f))
    return got


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
def test_cornell(device):
    """40 x 24 x 3: 45 full waves through the brute-force kernel with the table in LDS"""
    _assert_case(device, "cornell", frames=3)


@pytest.mark.parametrize("name,W,H,frames", [("cornell", 5, 13, 5), ("from_behind", 5, 13, 5), ("cornell", 1, 1, 4)])
def test_partial_waves(device, name, W, H, frames):
    """325 samples are five waves and five lanes (from behind the box with misses among them), four samples a single wave of four lanes"""
    _assert_case(device, name, W, H, frames)


def test_stripes(device):
    """stripe_rows = 5, n_ranks = 3, rank = 1: uneven stripes (rows 5-9 and 20-23), global pixel ids in the seeds"""
    _assert_case(device, "cornell", stripe_rows=5, n_ranks=3, rank=1)


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_every_search_on_the_box(device, quad, accel):
    """the packed filter and independent triangles, brute force and the LBVH over the box's 36 triangles"""
    with options(device, QUAD_FILTER=quad, ACCEL=accel):
        _assert_case(device, "cornell")


@pytest.mark.parametrize("name", ["soup", "with_big"])
def test_lbvh(device, name):
    """2 000 and 1 064 triangles take the LBVH (PT_OPT_ACCEL = 0); with_big fills the table of big triangles beside the hierarchy"""
    _assert_case(device, name)


@pytest.mark.parametrize("search,name,accel", fc.SLAB_FORMS, ids=[f[0] for f in fc.SLAB_FORMS])
def test_unbounded_scene_that_shades(device, search, name, accel):
    """pt_feature_kernel<false, ..> over the table in LDS and the tiled one, pt_feature_bvh_kernel<false, ..>: the boxes beside one
    triangle that lifts the scene over PT_DET_BOUND_MAX (scenes.slab), all four outputs; the slab's material shows in half the samples
    (tests/test_features_cpu.py)"""
    with options(device, QUAD_FILTER=0, ACCEL=accel):
        _assert_case(device, name, fc.SLAB_W, fc.SLAB_H)


def test_brute_force_equals_the_lbvh(device):
    """PT_OPT_ACCEL = 1 on the soup: the tiled brute-force kernel, the LBVH's samples and the oracle's"""
    want = _render(device, "soup")
    with options(device, ACCEL=1):
        got = _assert_case(device, "soup")
    for f in fo.FEATURES:
        assert_fb_equal(got[f], want[f], "brute force against the LBVH: %s" % f)


@pytest.mark.parametrize("name", ["odd_materials", "other_type", "from_behind", "non_finite"])
def test_edges(device, name):
    """ids outside the table and odd albedos, materials of neither type, the box from behind, triangles that are not finite and a
    normal that overflows to NaN"""
    got = _assert_case(device, name)
    if name == "non_finite":
        assert np.isnan(got["normal"]).any() and np.isnan(got["depth"]).any()


def test_lens(device):
    """R = 0.05, F = 6 at 40 x 24 x 3: the lens composes through the sample start; with the LBVH, too, where rays start off the eye"""
    _assert_case(device, "lens", frames=3)
    with options(device, ACCEL=2):
        _assert_case(device, "lens", frames=3)


def test_frame_begin_numbers_the_frames(device):
    """frames 7 and 8 alone equal frames 7 and 8 of a nine-frame call from 0"""
    whole = _render(device, "cornell", frames=9)
    part = _render(device, "cornell", frames=2, frame_begin=7)
    want = fc.oracle("cornell", frames=2, frame_begin=7)
    for f in fo.FEATURES:
        assert_fb_equal(part[f], whole[f][7:9], f)
        assert_fb_equal(part[f], getattr(want, f), f)


def test_outputs_left_out(device):
    """every subset of the outputs: those given equal the all-four call's, those left out are not written, no guard word moves"""
    b = Features(device, "cornell")
    try:
        assert b.call(b.params()) == shim.PT_OK
        want = {f: b.read(f)[0].copy() for f in fo.FEATURES}
        for k in range(1, 4):
            for which in itertools.combinations(fo.FEATURES, k):
                b.fill()
                assert b.call(b.params(), which) == shim.PT_OK, which
                _assert_samples(b, want, str(which), which)
                b.assert_untouched([f for f in fo.FEATURES if f not in which])
    finally:
        b.release()


def test_no_triangles(device):
    """num_triangles = 0 writes misses: zeros everywhere"""
    got = _render(device, "empty")
    for f in fo.FEATURES:
        assert not got[f].view(np.uint32).any(), f
    b = Features(device, "cornell")   # ... and with a scene in the buffer
    try:
        assert b.call(b.params(num_triangles=0)) == shim.PT_OK
        for f in fo.FEATURES:
            assert not b.read(f)[0].view(np.uint32).any(), f
    finally:
        b.release()


@pytest.mark.parametrize("name,accel", [("cornell", 1), ("soup", 0), ("lens", 1)])
def test_identity_with_camera_rays_and_queries(device, name, accel):
    """oracle-free, per frame: t, |normal| (the sign bit masked) and materials[clamp(id)].albedo equal pt_camera_rays ->
    pt_intersect_rays(PT_QUERY_CLOSEST) on the device; brute force and LBVH"""
    from oclpathtracer_amd.query import RayCaster

    tris, mats, cam = fc.case(name)
    with options(device, ACCEL=accel):
        got = _render(device, name, frames=3)
        caster = RayCaster(device, tris)
        try:
            for frame in range(3):
                hits = caster.closest(caster.camera_rays(fc.W, fc.H, frame, cam))
                hit = hits["tri"] >= 0
                assert 0 < int(hit.sum()) < len(hit)
                assert np.array_equal(got["depth"][frame][:, 1] == 1.0, hit)
                assert np.array_equal(got["depth"][frame][hit, 0].view(np.uint32), hits["t"][hit].view(np.uint32)), "t"
                assert np.array_equal(got["normal"][frame][hit].view(np.uint32) & 0x7fffffff,
                                      np.ascontiguousarray(hits["n"][hit]).view(np.uint32) & 0x7fffffff), "|normal|"
                mid = np.clip(hits["material"][hit], 0, len(mats) - 1)
                assert np.array_equal(got["albedo"][frame][hit].view(np.uint32), np.ascontiguousarray(mats["albedo"][mid, :3]).view(np.uint32))
                for f in fo.FEATURES:
                    assert not got[f][frame][~hit].view(np.uint32).any(), f
        finally:
            caster.release()


# ---- FeatureRenderer ---------------------------------------------------------------------------------------------------------------
def _assert_records_equal(got, want, what):
    for name in mom.MOMENTS_DTYPE.names:
        g, w = got[name], want[name]
        same = g.view(np.uint64) == w.view(np.uint64) if g.dtype == np.float64 else g == w
        assert same.all(), "%s: %s differs at %s" % (what, name, np.argwhere(~same)[:4].tolist())


@pytest.mark.parametrize("name", ["cornell", "non_finite"])
def test_feature_renderer(device, name):
    """render(5) through a workspace of two frames (calls of 2, 2 and 1 frames): the moments of every feature equal the restatement of
    pt_sample_moments over the oracle's samples bit for bit, mean and variance the restatement of pt_moments_resolve; then two more
    frames go on from there"""
    from oclpathtracer_amd.features import FEATURES, FeatureRenderer

    tris, mats, cam = fc.case(name)
    want = fc.oracle(name, frames=7)
    r = FeatureRenderer(device, tris, mats, fc.W, fc.H, features=FEATURES, camera=cam, stripe_rows=1, workspace_frames=2)
    try:
        for done in (5, 7):
            r.render(done - r.frames_done)
            assert r.frames_done == done
            for f in FEATURES:
                m = mom.accumulate(getattr(want, f)[:done])
                _assert_records_equal(r.moments(f), m, "%s after %d frames" % (f, done))
                mean, v = mom.resolve(m)
                assert np.array_equal(r.mean(f).view(np.uint64), mean.view(np.uint64)), f
                var, n = r.variance(f)
                assert_fb_equal(var, mom.noise_map(m)["var"], "variance of " + f)
                assert np.array_equal(n, m["n"])
        last = r.read_samples("depth", 2)   # the last call was frames 5 and 6
        assert_fb_equal(last, want.depth[5:7], "the workspace")
        t, cover = r.depth()
        m = mom.accumulate(want.depth)
        hits = m["sum"][:, 1]
        assert np.array_equal(cover, np.where(m["n"] > 0, hits / np.maximum(m["n"], 1), 0.0))
        assert np.array_equal(t[hits > 0], (m["sum"][:, 0] / np.where(hits > 0, hits, 1.0))[hits > 0]) and not t[hits == 0].any()
        if name == "non_finite":
            assert int(r.moments("normal")["rejected"].sum()) > 100 and int(r.moments("albedo")["rejected"].sum()) == 0
        r.render(1, 0)                      # frame 0 starts afresh
        _assert_records_equal(r.moments("albedo"), mom.accumulate(want.albedo[:1]), "after a restart")
        with pytest.raises(ValueError):
            r.render(1, 5)
        only = FeatureRenderer(device, tris, mats, 8, 8, features=("depth",))
        try:
            with pytest.raises(KeyError):
                only.moments("albedo")
        finally:
            only.release()
        with pytest.raises(ValueError):
            FeatureRenderer(device, tris, mats, 8, 8, features=("depth", "colour"))
    finally:
        r.release()


def test_feature_renderer_of_a_renderer_and_tensors(device, cornell):
    """Renderer.feature_renderer shares the renderer's buffers; the default features; set_camera restarts; variance as a device tensor"""
    import torch

    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    lens = fc.case("lens")[2]
    parent = Renderer(device, tris, mats, fc.W, fc.H, stripe_rows=1)
    r = parent.feature_renderer(workspace_frames=3)
    try:
        assert r.features == ("albedo", "normal", "depth") and r.tbuf is parent.tbuf and r.mbuf is parent.mbuf
        r.render(3)
        want = fc.oracle("cornell", frames=3)
        _assert_records_equal(r.moments("normal"), mom.accumulate(want.normal), "shared buffers")
        var, n = r.variance("depth")
        t = r.variance("depth", as_tensor=True)
        torch.cuda.synchronize()
        rec = t.cpu().numpy()
        assert_fb_equal(rec[:, :3], var, "the tensor's variance")
        assert np.array_equal(np.ascontiguousarray(rec[:, 3]).view(np.uint32), n)
        r.set_camera(lens)
        assert r.frames_done == 0
        r.render(3)
        _assert_records_equal(r.moments("depth"), mom.accumulate(fc.oracle("lens", frames=3).depth), "after set_camera")
    finally:
        r.release()
        parent.release()


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors(device):
    """every error comes with its code before anything is enqueued, and the outputs stay untouched"""
    b = Features(device, "cornell")
    W, H = b.W, b.H
    try:
        cases = [(dict(width=0), E_INV), (dict(height=-1), E_INV), (dict(frame_begin=-1), E_INV), (dict(frame_count=-1), E_INV),
                 (dict(num_triangles=-1), E_INV), (dict(num_materials=0), E_INV), (dict(stripe_rows=0), E_INV), (dict(n_ranks=0), E_INV),
                 (dict(rank=1), E_INV), (dict(rank=-1), E_INV), (dict(frame_begin=0x7fffffff, frame_count=1), E_INV),
                 (dict(width=65536, height=32768), E_INV),
                 (dict(num_triangles=len(b.tris) + 1), E_RANGE), (dict(num_materials=len(b.mats) + 1), E_RANGE),
                 (dict(width=W + 16), E_RANGE), (dict(frame_count=b.frames + 1), E_RANGE),
                 (dict(width=32768, height=32768, frame_count=2), E_RANGE)]            # 2^31 samples
        cases += [(dict(reserved=k), E_INV) for k in range(7)]
        for kw, code in cases:
            assert b.call(b.params(**kw)) == code, kw
        p = b.params()
        assert b.call(None) == E_INV
        assert b.call(p, tb=None) == E_INV and b.call(p, mb=None) == E_INV
        assert b.call(p, which=()) == E_INV                                           # at least one output
        bad = shim.Camera()
        b.lib.pt_camera_reference(ctypes.byref(bad))
        bad.fov_y_deg = 180.0
        assert b.call(p, cam=bad) == E_INV
        bad.fov_y_deg, bad.reserved[3] = 60.0, 1
        assert b.call(p, cam=bad) == E_INV
        for f in fo.FEATURES:
            small = adl.Buffer(device, b.words - 1, np.float32)
            try:
                assert b.call(p, **{f: small}) == E_RANGE, f                          # a float short
            finally:
                small.release()
        other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
        ob = adl.Buffer(other, b.words, np.float32)
        big = adl.Buffer(device, 8 * b.words + 64, np.uint8)
        try:
            assert b.call(p, normal=ob) == E_INV                                      # a buffer of another device

            def wrap(off, nbytes, base=big):                                          # sub-ranges of one allocation
                w = adl.Buffer()
                w.setRawPtr(device, base.m_ptr + off, nbytes)
                return w
            nb = 4 * b.words
            odd, first, into = wrap(2, nb), wrap(0, nb), wrap(nb - 4, nb)
            over_t, over_m = wrap(64, 64, b.tb), wrap(0, 64, b.mb)
            try:
                assert b.call(p, depth=odd) == E_INV                                  # not 4-byte aligned
                assert b.call(p, albedo=first, emission=into) == E_INV                # two outputs overlap
                assert b.call(p, albedo=first, emission=first) == E_INV               # ... or are one buffer
                assert b.call(b.params(frames=0), albedo=first, emission=into) == shim.PT_OK   # (nothing to write: nothing overlaps)
                one = b.params(width=1, height=1, frames=1)
                assert b.call(one, normal=over_t) == E_INV                            # an output inside the triangles
                assert b.call(one, depth=over_m) == E_INV                             # ... inside the materials
            finally:
                for w in (odd, first, into, over_t, over_m):
                    w.release()
        finally:
            big.release()
            ob.release()
            adl.DeviceUtils.deallocate(other)
        b.assert_untouched()
        assert b.call(p) == shim.PT_OK                                                # and the call still works
        _assert_samples(b, fc.oracle("cornell"), "after the errors")
    finally:
        b.release()


# ---- the harness --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(), ("--lens", "0.05,6")])
def test_harness_features(lens):
    """raytrace_test --only Features [--lens R,F]: renders, prints coverage and mean depth, cross-checks frame 0 on the device"""
    import os
    import re
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, "oclpathtracer_amd", "raytrace_test")
    scene_path = os.path.join(ROOT, "oclpathtracer_amd", "data", "cornellbox.bin")
    r = subprocess.run([exe, "--only", "Features", *lens, "--dim", "48", "--frames", "5", "--scene", scene_path], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 1 and "FAILED" not in r.stdout, r.stdout
    assert "frame 0 equals pt_camera_rays + pt_intersect_rays on 2304 pixels" in r.stdout
    m = re.search(r"coverage ([0-9.]+), mean depth ([0-9.]+) over (\d+) hits of (\d+) samples, 0 rejected", r.stdout)
    assert m, r.stdout
    assert 0.5 < float(m.group(1)) <= 1.0 and 4.0 < float(m.group(2)) < 12.0 and int(m.group(4)) == 48 * 48 * 5
