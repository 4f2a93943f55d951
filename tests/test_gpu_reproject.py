"""pt_reproject on the device, bit for bit -- the moment records and the info map -- against the numpy restatement
(tests/reproject_oracle.py, which tests/test_reproject_cpu.py examines on its own): synthetic records of a two-wall scene under five
camera pairs at image sizes that are no multiple of a tile and cross one, Cornell-box records from the CPU oracles, every parameter's
ends, both kernel forms, the asynchronous call that allocates nothing, the argument errors, TemporalAccumulator end to end and the
harness line."""
import ctypes
import re

import numpy as np
import pytest

import denoise_oracle as do
import moments_oracle as mo
import reproject_cases as rc
import reproject_oracle as ro
from conftest import assert_fb_equal
from gpu_support import harness_ppm, options
from oclpathtracer_amd import adl, shim

pytestmark = pytest.mark.gpu

F = np.float32
E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
FRAMES = 12
SHAPES = [(1, 1), (2, 3), (5, 4), (67, 35), (130, 9)]
# (previous camera, current camera): equal; a small shift; a pan that pushes a band of pixels out of the old image; a changed field of
# view; the old camera turned away, so that dz <= 0 everywhere
PAIRS = [("ref", "ref"), ("ref", "shifted"), ("ref", "panned"), ("ref", "wide"), ("away", "ref")]
_CASES = {}


def _view(cam, w, h, rng):
    """(colour, normal, depth) records of what `cam` sees of a world of two walls -- the back wall z = -1.5 and, in front of it for
    x > 0.5, a nearer wall z = 1 -- so that depths are consistent between cameras and taps do survive; a ray that meets neither (a
    camera turned away) has no coverage.  FRAMES samples a pixel, some of them missing"""
    n = w * h
    d = cam.derive().astype(np.float64)
    eye, view, hol, up, angle = d[0:3], d[3:6], d[6:9], d[9:12], d[12]
    x, y = np.arange(n) % w, np.arange(n) // w
    xs = (2.0 * (x + 0.5) / w - 1.0) * angle * (w / h)
    ys = (1.0 - 2.0 * (y + 0.5) / h) * angle
    wv = hol[None] * xs[:, None] + up[None] * ys[:, None] + view[None]
    dirv = wv / np.sqrt((wv * wv).sum(axis=1))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t_near = (1.0 - eye[2]) / dirv[:, 2]
        near = (t_near > 0) & (eye[0] + t_near * dirv[:, 0] > 0.5)
        t = np.where(near, t_near, (-1.5 - eye[2]) / dirv[:, 2])
    hit = t > 0
    t = np.where(hit, t, 0.0)
    cos = np.abs(dirv[:, 2])
    jit = lambda a, s: (a[None] + rng.uniform(-s, s, (FRAMES,) + a.shape)).astype(F)
    dep = np.zeros((FRAMES, n, 3), F)
    dep[..., 0], dep[..., 1], dep[..., 2] = jit(t, 0.002), 1.0, jit(cos, 0.01)
    nrm = jit(np.repeat(np.array([[0.0, 0.0, 1.0]]), n, 0), 0.02)
    col = rng.uniform(0.2, 1.8, (FRAMES, n, 3)).astype(F) * np.where(near, 4.0, 1.0).astype(F)[None, :, None]
    missed = (rng.uniform(size=(FRAMES, n)) < 0.1) | ~hit[None, :]                  # partial coverage: a sample that missed
    dep[missed] = 0.0
    nrm[missed] = 0.0
    count = rng.integers(1, FRAMES + 1, n)                                          # history lengths 1 .. FRAMES: above and below a cap of 5
    col[np.arange(FRAMES)[:, None] >= count[None, :]] = np.nan                      # (the frames beyond a pixel's count are rejected)
    return col, nrm, dep


def synthetic(w, h, prev, cur):
    """the five record arrays of pt_reproject for a w x h image under the camera pair, made once and shared read-only: _view of each
    camera, and sprinkled over them pixels with n = 0 (zero records), only rejected samples, n = 1, no coverage, a zero normal, a NaN
    normal record, a depth of 1e30 (the projection overflows) and a history of one bright sample among dark ones"""
    key = (w, h, prev, cur)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * w + h + 7 * PAIRS.index((prev, cur)))
    cams = rc.cameras()
    n = w * h
    pick = lambda p: rng.uniform(size=n) < p
    pcol, pnrm, pdep = _view(cams[prev], w, h, rng)
    _, cnrm, cdep = _view(cams[cur], w, h, rng)
    rejected, one = pick(0.03), pick(0.04)
    pcol[:, rejected] = np.nan
    pcol[1:, one] = np.inf
    pcol[0, one] = (0.75, 0.5, 0.25)
    spike = pick(0.04)                                                              # one bright sample among dark ones: the noise test
    pcol[:, spike] *= F(0.001)
    pcol[0, spike] = (900.0, 700.0, 500.0)
    for nrm, dep in ((pnrm, pdep), (cnrm, cdep)):
        never = pick(0.04)
        dep[:, never] = 0.0
        nrm[:, never] = 0.0
        nrm[:, pick(0.04)] = 0.0
    colour = mo.accumulate(pcol)
    empty = pick(0.03)
    colour[empty] = 0                                                               # n = 0 and nothing rejected
    recs = [colour] + [mo.accumulate(a) for a in (pnrm, pdep, cnrm, cdep)]
    nan_p, nan_c, far = pick(0.02), pick(0.02), pick(0.02)
    recs[1]["sum"][nan_p] = np.nan
    recs[3]["sum"][nan_c] = np.nan
    recs[4]["sum"][far, 0] = 1e30 * recs[4]["sum"][far, 1]
    if n > 100:
        assert (colour["n"] == 0).any() and (colour["rejected"] == FRAMES).any() and (colour["n"] == 1).any()
        assert (colour["n"] > 5).any() and ((colour["n"] > 1) & (colour["n"] < 5)).any()
        if prev != "away":
            quiet = ro.reproject(*recs, w, h, cams[prev], cams[cur], max_noise=0.0)[0]["n"] > 0
            noisy = ro.reproject(*recs, w, h, cams[prev], cams[cur], max_noise=0.5)[0]["n"] > 0
            assert (quiet & ~noisy).any() and not (noisy & ~quiet).any()          # the noise test sets some taps aside
        for nrm, dep in ((recs[1], recs[2]), (recs[3], recs[4])):
            if dep["sum"][:, 1].any():
                assert (dep["sum"][:, 1] == 0).any() and ((nrm["n"] > 0) & (nrm["sum"] == 0).all(axis=1)).any()
            assert np.isnan(nrm["sum"]).any()
        covered = recs[4]["sum"][:, 1] > 0
        assert (recs[4]["sum"][covered, 0] > 1e29).any()
        out, info = ro.reproject(*recs, w, h, cams[prev], cams[cur])
        took = out["n"] > 0
        if prev == "away":
            assert not took.any() and not info.any()                                # dz <= 0 everywhere: nothing reaches step 6
        else:
            assert took.any() and (~took & covered).any() and (info[covered, 2] > 0).any()
        if (prev, cur) == ("ref", "panned"):
            assert (covered & ~info.any(axis=1)).sum() >= h                         # a band of pixels left the old image
    for a in recs:
        a.setflags(write=False)
    _CASES[key] = recs
    return recs


def assert_records_equal(got, want, what):
    """moment records bit for bit: raw bytes, or -- where a sum is a NaN, whose payload differs between the machines -- field by field"""
    if got.tobytes() == want.tobytes():
        return
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["rejected"], want["rejected"]), what
    for f in ("sum", "sum2"):
        g, w = got[f].reshape(-1), want[f].reshape(-1)
        gn, wn = np.isnan(g), np.isnan(w)
        assert np.array_equal(gn, wn), what
        assert np.array_equal(g.view(np.uint64)[~gn], w.view(np.uint64)[~wn]), what


class Raw:
    """The buffers of raw calls of pt_reproject on one set of records; both outputs start as sentinels and have a guard behind them"""

    NAMES = ("prev_colour", "prev_normal", "prev_depth", "cur_normal", "cur_depth")

    def __init__(self, device, w, h, recs, prev, cur, pad=3):
        self.device, self.lib, self.w, self.h, self.recs = device, shim.load(), w, h, recs
        cams = rc.cameras()
        self.cams = (cams[prev], cams[cur])
        self.structs = tuple(c.to_struct() for c in self.cams)
        n = w * h
        self.bufs = {}
        for name, rec in zip(self.NAMES, recs):
            b = adl.Buffer(device, n * 56, np.uint8)
            b.write(np.ascontiguousarray(rec).view(np.uint8), n * 56)
            self.bufs[name] = b
        self.bufs["scratch"] = adl.Buffer(device, self.lib.pt_reproject_scratch_bytes(w, h), np.uint8)
        self.bufs["out"] = adl.Buffer(device, (n + pad) * 56, np.uint8)
        self.bufs["info"] = adl.Buffer(device, n + pad, adl.float4)
        self.out_sentinel = np.full((n + pad) * 56, 0xA5, np.uint8)
        self.info_sentinel = np.full((n + pad, 4), F(-7.25), F)
        self.reset()

    def reset(self):
        self.bufs["out"].write(self.out_sentinel, len(self.out_sentinel))
        self.bufs["info"].write(self.info_sentinel, len(self.info_sentinel))

    def call(self, p, ev=None, cams=None, **over):
        """pt_reproject; `over`: a buffer replaced by name (None: a NULL handle); cams: the two pt_camera structs (None: NULL)"""
        hs = dict(self.bufs)
        hs.update(over)
        h = lambda b: b._h if b is not None else None
        pc, cc = self.structs if cams is None else cams
        ref = lambda s: ctypes.byref(s) if s is not None else None
        return self.lib.pt_reproject(self.device._h, *[h(hs[k]) for k in self.NAMES], h(hs["scratch"]), h(hs["out"]), h(hs["info"]),
                                     ctypes.byref(p) if p is not None else None, ref(pc), ref(cc), ev)

    def read(self):
        out, info = np.zeros_like(self.out_sentinel), np.zeros_like(self.info_sentinel)
        self.bufs["out"].read(out, len(out))
        self.bufs["info"].read(info, len(info))
        self.device.waitForCompletion()
        return out, info

    def untouched(self):
        out, info = self.read()
        return np.array_equal(out, self.out_sentinel) and np.array_equal(info, self.info_sentinel)

    def check(self, what, normals=True, info=True, **kw):
        """one call under `kw` against the restatement: records and info bit for bit, the guards untouched"""
        n = self.w * self.h
        self.reset()
        over = {} if normals else dict(prev_normal=None, cur_normal=None)
        if not info:
            over["info"] = None
        assert self.call(params(self.w, self.h, **kw), **over) == shim.PT_OK, self.lib.pt_last_error()
        got, got_info = self.read()
        r = self.recs
        want, want_info = ro.reproject(r[0], r[1] if normals else None, r[2], r[3] if normals else None, r[4], self.w, self.h, *self.cams, **kw)
        assert_records_equal(got[:n * 56].view(mo.MOMENTS_DTYPE), want, what)
        assert np.array_equal(got[n * 56:], self.out_sentinel[n * 56:]), "%s: written behind the records" % what
        if info:
            assert_fb_equal(got_info[:n], want_info, what)
            assert np.array_equal(got_info[n:], self.info_sentinel[n:]), "%s: written behind the info" % what
        else:
            assert np.array_equal(got_info, self.info_sentinel), "%s: info written though NULL" % what
        return want, want_info

    def release(self):
        for b in self.bufs.values():
            b.release()


def params(w, h, **kw):
    p = shim.ReprojectParams()
    v = dict(ro.DEFAULTS)
    v.update(kw)
    p.width, p.height = w, h
    for k, x in v.items():
        if k == "reserved":
            p.reserved[x] = 1
        else:
            setattr(p, k, x)
    return p


@pytest.mark.parametrize("prev,cur", PAIRS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_parity(device, w, h, prev, cur):
    """every shape under every camera pair, at the default cap, a cap of 5 -- below and above the histories -- and without normals"""
    r = Raw(device, w, h, synthetic(w, h, prev, cur), prev, cur)
    try:
        r.check("%dx%d %s -> %s" % (w, h, prev, cur))
        r.check("%dx%d %s -> %s, cap 5" % (w, h, prev, cur), max_history=5)
        r.check("%dx%d %s -> %s, no normals" % (w, h, prev, cur), normals=False)
    finally:
        r.release()


@pytest.mark.parametrize("move", ["shifted", "panned"])
def test_cornell_records(device, cornell, move):
    """records of the CPU oracles at 33 x 17: an 8-frame history and features under the reference camera, one feature frame under the
    moved one"""
    tris, mats = cornell
    w, h = 33, 17
    pf = rc.feature_records(tris, mats, w, h, "ref", 8)
    cf = rc.feature_records(tris, mats, w, h, move, 1, 8)
    recs = [rc.colour_records(tris, mats, w, h, "ref", 0, 8), pf["normal"], pf["depth"], cf["normal"], cf["depth"]]
    r = Raw(device, w, h, recs, "ref", move)
    try:
        want, info = r.check("cornell %s" % move)
        assert (want["n"] == 8).sum() > 250 and ((want["n"] == 0) & (cf["depth"]["sum"][:, 1] > 0)).any()
        r.check("cornell %s, cap 3" % move, max_history=3)
    finally:
        r.release()


def test_parameters(device):
    w, h = 67, 35
    r = Raw(device, w, h, synthetic(w, h, "ref", "shifted"), "ref", "shifted")
    try:
        base, _ = r.check("defaults")
        for cap in (0, 1, 5, 0x7fffffff):
            want, info = r.check("max_history %d" % cap, max_history=cap)
            assert want["n"].max() == min(cap, FRAMES)
        assert not r.check("max_history 0 again", max_history=0)[0]["n"].any()
        r.check("no normals", normals=False)
        r.check("no info", info=False)
        loose, _ = r.check("cos_min 0", cos_min=0.0)
        tight, _ = r.check("cos_min 1", cos_min=1.0)
        assert (loose["n"] > 0).sum() >= (base["n"] > 0).sum() > (tight["n"] > 0).sum()
        any_w, _ = r.check("min_weight 0", min_weight=0.0)
        most, _ = r.check("min_weight 0.99", min_weight=0.99)
        assert (any_w["n"] > 0).sum() > (base["n"] > 0).sum() > (most["n"] > 0).sum()
        # a tolerance that rejects everything -- but the pixels whose depth of 1e30 overflows the projection to r = inf, where both
        # sides of the depth test are infinite and IEEE's inf <= inf holds
        off, _ = r.check("max_noise 0: no noise test", max_noise=0.0)
        strict, _ = r.check("max_noise 1e-6", max_noise=1e-6)
        lax, _ = r.check("max_noise 1e30", max_noise=1e30)
        assert (off["n"] > 0).sum() > (base["n"] > 0).sum() > (strict["n"] > 0).sum() and lax.tobytes() == off.tobytes()
        none, info = r.check("tol_z rejects everything", tol_z=1e-30)
        far = r.recs[4]["sum"][:, 0] > 1e29
        assert not none["n"][~far].any() and not info[~far, 2:].any() and info[:, :2].any()
        some, _ = r.check("tol_z rejects most", tol_z=1e-3)
        wide, _ = r.check("tol_z accepts everything", tol_z=1e30)
        assert 0 < (some["n"] > 0).sum() < (base["n"] > 0).sum() <= (wide["n"] > 0).sum()
    finally:
        r.release()


@pytest.mark.parametrize("w,h", [(67, 35), (130, 9)])
def test_both_forms(device, w, h):
    """PT_OPT_REPROJECT_FORM 1 (one kernel over the records), 2 (a prepare pass first) and 0 (the shipped choice): the same bits"""
    lib = shim.load()
    assert lib.pt_device_get_option(device._h, shim.PT_OPT_REPROJECT_FORM) == 0
    assert lib.pt_device_set_option(device._h, shim.PT_OPT_REPROJECT_FORM, 3) == E_INV and lib.pt_device_set_option(device._h, shim.PT_OPT_REPROJECT_FORM, -1) == E_INV
    for prev, cur in (("ref", "shifted"), ("ref", "panned")):
        r = Raw(device, w, h, synthetic(w, h, prev, cur), prev, cur)
        try:
            for mode in (1, 2, 0):
                with options(device, REPROJECT_FORM=mode):
                    assert lib.pt_device_get_option(device._h, shim.PT_OPT_REPROJECT_FORM) == mode
                    r.check("form %d" % mode)
                    r.check("form %d, no normals, cap 5" % mode, normals=False, max_history=5)
                    r.check("form %d, no info" % mode, info=False, min_weight=0.0)
                    r.check("form %d, no noise test" % mode, max_noise=0.0)
        finally:
            r.release()


def test_asynchronous_and_allocates_nothing(device):
    """three calls with an event each: the handle's workspace and the device's memory in use stand still, the event completes and has
    measured the call, and the inputs read back unchanged"""
    lib = shim.load()
    w, h = 130, 9
    n = w * h
    recs = synthetic(w, h, "ref", "shifted")
    r = Raw(device, w, h, recs, "ref", "shifted")
    ev = adl.SyncObject(device)
    try:
        want, want_info = r.check("warm")
        ws, used = lib.pt_device_workspace_memory(device._h), lib.pt_device_used_memory(device._h)
        p = params(w, h)
        for i in range(3):
            assert r.call(p, ev=ev._h) == shim.PT_OK
            assert lib.pt_device_workspace_memory(device._h) == ws and lib.pt_device_used_memory(device._h) == used
        ev.waitForCompletion()
        assert ev.isComplete() and ev.getExecutionTimeNanoseconds() > 0
        got, got_info = r.read()
        assert_records_equal(got[:n * 56].view(mo.MOMENTS_DTYPE), want, "after three calls")
        assert_fb_equal(got_info[:n], want_info, "after three calls")
        back = np.zeros(n * 56, np.uint8)
        for name, rec in zip(Raw.NAMES, recs):
            r.bufs[name].read(back, n * 56)
            device.waitForCompletion()
            assert back.tobytes() == rec.tobytes(), "%s was written" % name
    finally:
        ev.release()
        r.release()


def test_argument_errors_leave_the_outputs_untouched(device):
    from oclpathtracer_amd.camera import Camera

    lib = shim.load()
    w, h = 5, 4
    n = w * h
    r = Raw(device, w, h, synthetic(w, h, "ref", "shifted"), "ref", "shifted")
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    ob = adl.Buffer(other, n * 56, np.uint8)
    big = adl.Buffer(device, 64 * 1024, np.uint8)
    SB = lib.pt_reproject_scratch_bytes(w, h)
    wraps = []

    def wrap(off, nbytes):
        b = adl.Buffer()
        b.setRawPtr(device, big.m_ptr + off, nbytes)
        wraps.append(b)
        return b

    try:
        ok = params(w, h)
        b = r.bufs
        assert lib.pt_reproject(None, *[b[k]._h for k in Raw.NAMES], b["scratch"]._h, b["out"]._h, b["info"]._h, ctypes.byref(ok), None, None, None) == E_INV
        assert r.call(None) == E_INV
        for name in ("prev_colour", "prev_depth", "cur_depth", "scratch", "out"):
            assert r.call(ok, **{name: None}) == E_INV, name
        assert r.call(ok, prev_normal=None) == E_INV and r.call(ok, cur_normal=None) == E_INV      # exactly one of the two normals
        for name in Raw.NAMES + ("scratch", "out", "info"):
            assert r.call(ok, **{name: ob}) == E_INV, name                                         # a buffer of another device
        for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(width=65536, height=32768), dict(max_history=-1), dict(reserved=0),
                   dict(reserved=8)):
            assert r.call(params(w, h, **kw)) == E_INV, kw
        for name, bads in (("tol_z", (0.0, -0.0, -1.0, float("nan"), float("inf"), 1e-50)), ("cos_min", (-0.5, 1.5, float("nan"), float("inf"))),
                           ("min_weight", (-0.5, 1.0, 2.0, float("nan"), float("inf"))), ("max_noise", (-0.5, float("nan"), float("inf")))):
            for bad in bads:
                assert r.call(params(w, h, **{name: bad})) == E_INV, (name, bad)
        # cameras: one pt_camera_derive rejects, and a lens
        flat = rc.cameras()["ref"].to_struct()
        flat.fov_y_deg = 180.0
        lens = Camera.reference().with_lens(0.05, focus_distance=3.0).to_struct()
        for bad in (flat, lens):
            assert r.call(ok, cams=(bad, r.structs[1])) == E_INV and r.call(ok, cams=(r.structs[0], bad)) == E_INV
        # too small: RANGE
        assert r.call(params(w + 1, h)) == E_RANGE
        for name in Raw.NAMES + ("out",):
            assert r.call(ok, **{name: wrap(0, n * 56 - 1)}) == E_RANGE, name
        assert r.call(ok, info=wrap(0, n * 16 - 1)) == E_RANGE and r.call(ok, scratch=wrap(0, SB - 1)) == E_RANGE
        # alignment
        for name in Raw.NAMES + ("out",):
            assert r.call(ok, **{name: wrap(4, n * 56)}) == E_INV, name
        assert r.call(ok, info=wrap(8, n * 16)) == E_INV and r.call(ok, scratch=wrap(8, SB)) == E_INV
        # overlap: of an input with an output, of the two outputs, of an output with the scratch, of two inputs
        assert r.call(ok, prev_colour=wrap(0, n * 56), out=wrap(n * 56 - 8, n * 56)) == E_INV
        assert r.call(ok, out=wrap(16384, n * 56), info=wrap(16384 + n * 56 - 16 - (n * 56 - 16) % 16, n * 16)) == E_INV
        assert r.call(ok, info=wrap(32768, n * 16), scratch=wrap(32768 + n * 16 - 16, SB)) == E_INV
        assert r.call(ok, prev_normal=b["cur_normal"]) == E_INV and r.call(ok, prev_depth=b["cur_depth"]) == E_INV
        assert r.call(ok, out=b["prev_colour"]) == E_INV
        assert r.untouched(), "an error touched an output"
        # (adjacent ranges are fine, and so are NULL cameras: the reference's)
        assert r.call(ok, prev_colour=wrap(0, n * 56), out=wrap(n * 56, n * 56), scratch=wrap(32768, SB), cams=(None, None)) == shim.PT_OK
        device.waitForCompletion()
    finally:
        for b in wraps:
            b.release()
        big.release()
        ob.release()
        r.release()
        adl.DeviceUtils.deallocate(other)


# ---- through the renderers -------------------------------------------------------------------------------------------------------
def _records(device, buf, n):
    rec = np.zeros(n, mo.MOMENTS_DTYPE)
    buf.read(rec.view(np.uint8), rec.nbytes)
    device.waitForCompletion()
    return rec


def test_temporal_accumulator_end_to_end(device, cornell):
    """Cornell 48 x 40, indirect illumination at B = 4, K = 1: render(8), move(shifted), render(2).  The moments are the restatement
    applied to the records read back before the move, plus the two new frames' samples -- frames 8 and 9 of the CPU oracle under the new
    camera: the renderer went on at its frame count --, and the denoiser takes them with the accumulator's features"""
    import indirect_oracle as io
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.denoise import Denoiser
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = cornell
    W, H = 48, 40
    n = W * H
    cams = rc.cameras()
    r = IndirectRenderer(device, tris, mats, W, H, max_bounces=4, light_samples=1, moments=True, stripe_rows=1)
    acc = d = None
    try:
        acc = r.temporal()
        assert not acc.info().any() and not acc.history().any()
        acc.render(8)
        assert r.frames_done == acc.features.frames_done == 8
        before = _records(device, r.mom, n)
        old = acc.features
        pf = {f: old.moments(f) for f in ("normal", "depth")}
        assert before["n"].max() == 8
        acc.move(cams["shifted"])
        assert acc.features is not old and r.frames_done == 8 and r.camera == cams["shifted"] and acc.features.frames_done == 9
        cf = {f: acc.features.moments(f) for f in ("normal", "depth")}
        assert cf["depth"]["n"].max() == 1
        want, want_info = ro.reproject(before, pf["normal"], pf["depth"], cf["normal"], cf["depth"], W, H, None, cams["shifted"])
        assert_records_equal(_records(device, r.mom, n), want, "the history after the move")
        assert_fb_equal(acc.info(), want_info, "info")
        assert np.array_equal(acc.history().reshape(-1), want["n"]) and (want["n"] == 8).sum() > 0.8 * n
        acc.render(2)
        assert r.frames_done == 10
        gid, frame = io.all_samples(W, H, 2, 8)
        new = io.samples(tris, mats, W, H, gid, frame, 1, 4, cam=cams["shifted"])[0].reshape(2, n, 3)
        merged = mo.accumulate(new, want)
        got = _records(device, r.mom, n)
        assert_records_equal(got, merged, "history plus two frames")
        assert got["n"].max() == 10 and got["n"].min() == 2
        assert_fb_equal(acc.mean(), mo.resolve(merged)[0].astype(F), "mean()")
        d = Denoiser(device, W, H)
        guides = [acc.features.moments(f) for f in ("albedo", "normal", "depth", "emission")]
        assert guides[2]["n"].max() == 3                                               # one frame at the move, two with the render
        assert_fb_equal(d.denoise(r.mom, acc.features), do.denoise(got, *guides, W, H), "denoised")
        # a second move, back: the history now has 10 and 2 samples a pixel
        acc.move(None)
        again = ro.reproject(got, guides[1], guides[2], acc.features.moments("normal"), acc.features.moments("depth"), W, H, cams["shifted"], None)[0]
        assert_records_equal(_records(device, r.mom, n), again, "the second move")
        for bad in (dict(), dict(moments=True, stripe_rows=8, n_ranks=2), dict(moments=True, camera=Camera.reference().with_lens(0.05, focus_distance=3.0))):
            two = DirectRenderer(device, tris, mats, W, H, **bad)
            try:
                with pytest.raises(ValueError):
                    two.temporal()
            finally:
                two.release()
        with pytest.raises(ValueError):
            acc.move(Camera.reference().with_lens(0.05, focus_distance=3.0))
    finally:
        for o in (d, acc):
            if o is not None:
                o.release()
        r.release()


# ---- the harness ----------------------------------------------------------------------------------------------------------------
_LINE = re.compile(r"^reproject: history pixels (\d+) of (\d+) mean_length (\S+)\n", re.M)


def test_harness_reproject(device, tmp_path, cornell):
    """raytrace_test --noise --reproject 0.3,0,0,6 (32 x 32, 12 frames) prints one line more than --noise alone and changes nothing
    else; its figures are those of TemporalAccumulator.history() for the same render and move"""
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.indirect import IndirectRenderer

    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain_out, name, plain_pixels = harness_ppm(tmp_path / "a", 32, 12, "IndirectIllumination", "--noise")
    out, rp_name, pixels = harness_ppm(tmp_path / "b", 32, 12, "IndirectIllumination", "--noise", "--reproject", "0.3,0,0,6")
    assert name == rp_name and np.array_equal(pixels, plain_pixels)
    assert _LINE.search(plain_out) is None and len(_LINE.findall(out)) == 1
    mask = lambda t: re.sub(r"in \d+\.\d+ s", "in # s", t).replace(str(tmp_path / "b"), "DIR").replace(str(tmp_path / "a"), "DIR")
    assert mask(_LINE.sub("", out)) == mask(plain_out)
    tris, mats = cornell
    r = IndirectRenderer(device, tris, mats, 32, 32, max_bounces=16, light_samples=1, stripe_rows=1, chunk_frames=8, moments=True)
    acc = None
    try:
        acc = r.temporal(max_history=6)
        acc.render(12)
        acc.move(Camera((0.3, 2.75, 4.0), (0.3, 2.75, 3.0)))
        hist = acc.history()
    finally:
        if acc is not None:
            acc.release()
        r.release()
    g = _LINE.search(out).groups()
    took = hist > 0
    assert int(g[0]) == took.sum() > 800 and int(g[1]) == 32 * 32
    assert abs(float(g[2]) - hist[took].mean()) <= 2e-9 * hist[took].mean() and hist.max() == 6
