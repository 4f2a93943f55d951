"""pt_denoise_spatial on the device, bit for bit -- all four channels -- against the numpy restatement (tests/denoise_spatial_oracle.py,
which tests/test_denoise_spatial_cpu.py examines on its own) through the raw C ABI: three sets of records at image sizes smaller than
the pool's halo, no multiple of a tile and cut by both borders, every `below` that changes which pixels are listed, every combination
of guides, both forms of the pool pass under both gathers of the levels, workgroups that leave early beside ones that do not, the
identity with pt_denoise, the asynchronous call that allocates nothing, the argument errors, the renderers end to end and the harness."""
import ctypes
import re

import numpy as np
import pytest

import denoise_oracle as do
import denoise_spatial_oracle as dso
import moments_oracle as mo
from conftest import assert_fb_equal
from gpu_support import harness_ppm, options
from oclpathtracer_amd import adl, shim
from test_gpu_denoise import FRAMES, params, synthetic

pytestmark = pytest.mark.gpu

F = np.float32
E_INV = shim.PT_ERR_INVALID
SHAPES = [(1, 1), (2, 3), (5, 4), (67, 35), (130, 9)]
BELOWS = [0, 1, 2, 3, 5, 2 ** 31 - 1]
LEVELS = [0, 1, 5]
SETS = ["synthetic", "one_frame", "mixed"]
_COLOUR = {}


def colour_of(name, w, h):
    """the colour records of a set, made once per size and shared read-only (the guides are synthetic(w, h)'s for every set):
    synthetic -- n in {0, 1, 4} and rejected-only pixels; one_frame -- every n = 1; mixed -- n in 1 .. 4 and a block of zero records"""
    if name == "synthetic":
        return synthetic(w, h)[0]
    if (name, w, h) not in _COLOUR:
        rng = np.random.default_rng(77 * w + h + len(name))
        n = w * h
        level = np.where(np.arange(n) % w * 3 < w, 0.4, 2.5).astype(F)
        s = (rng.uniform(0.2, 1.8, (FRAMES, n, 3)).astype(F) * level[None, :, None]).astype(F)
        s[:, rng.uniform(size=n) < 0.05] *= F(30.0)                                     # fireflies
        if name == "one_frame":
            col = mo.accumulate(s[:1])
            assert (col["n"] == 1).all()
        else:
            keep = rng.integers(1, FRAMES + 1, n)
            for f in range(FRAMES):
                s[f, keep <= f] = np.nan                                                # rejected: n = keep
            col = mo.accumulate(s)
            x, y = np.arange(n) % w, np.arange(n) // w
            col[(x >= w // 3) & (x < w // 3 + 5) & (y >= h // 2) & (y < h // 2 + 4)] = 0     # a block of zero records
            if n > 100:
                assert set(np.unique(col["n"])) == {0, 1, 2, 3, 4}
        col.setflags(write=False)
        _COLOUR[(name, w, h)] = col
    return _COLOUR[(name, w, h)]


def spatial(below, reserved=None):
    sp = shim.DenoiseSpatialParams()
    sp.below = below
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


class Raw:
    """The buffers of raw calls of pt_denoise_spatial (and pt_denoise) on one case; `out` starts as a sentinel and has a guard behind it"""

    def __init__(self, device, w, h, colour, pad=3):
        self.device, self.lib, self.w, self.h = device, shim.load(), w, h
        self.colour, self.guides = colour, synthetic(w, h)[1]
        n = w * h
        self.bufs = []
        for rec in [self.colour] + self.guides:
            b = adl.Buffer(device, n * 56, np.uint8)
            b.write(np.ascontiguousarray(rec).view(np.uint8), n * 56)
            self.bufs.append(b)
        self.scratch = adl.Buffer(device, self.lib.pt_denoise_scratch_bytes(w, h), np.uint8)
        self.out = adl.Buffer(device, n + pad, adl.float4)
        self.sentinel = np.full((n + pad, 4), F(-7.25), F)
        self.reset()

    def reset(self):
        self.out.write(self.sentinel, len(self.sentinel))

    def handles(self, mask):
        return [self.bufs[0]._h] + [self.bufs[1 + i]._h if mask >> i & 1 else None for i in range(4)] + [self.scratch._h, self.out._h]

    def call(self, p, sp, mask=15, ev=None):
        return self.lib.pt_denoise_spatial(self.device._h, *self.handles(mask), ctypes.byref(p) if p is not None else None,
                                           ctypes.byref(sp) if sp is not None else None, ev)

    def plain(self, p, mask=15):
        """pt_denoise on the same buffers: the image"""
        assert self.lib.pt_denoise(self.device._h, *self.handles(mask), ctypes.byref(p), None) == shim.PT_OK, self.lib.pt_last_error()
        return self.read()[:self.w * self.h]

    def read(self):
        got = np.zeros_like(self.sentinel)
        self.out.read(got, len(got))
        self.device.waitForCompletion()
        return got

    def want(self, below, mask=15, **kw):
        g = [self.guides[i] if mask >> i & 1 else None for i in range(4)]
        return dso.denoise(self.colour, *g, self.w, self.h, below, **kw).reshape(self.w * self.h, 4)

    def check(self, what, below, mask=15, want=None, **kw):
        """one call under `kw` against the restatement: the image bit for bit, the guard untouched"""
        n = self.w * self.h
        assert self.call(params(self.w, self.h, **kw), spatial(below), mask) == shim.PT_OK, self.lib.pt_last_error()
        got = self.read()
        assert_fb_equal(got[:n], self.want(below, mask, **kw) if want is None else want, what)
        assert np.array_equal(got[n:], self.sentinel[n:]), "%s: written behind the image" % what
        return got[:n]

    def release(self):
        for b in self.bufs + [self.scratch, self.out]:
            b.release()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_parity(device, w, h, name):
    """every shape and record set at every `below` and level count"""
    r = Raw(device, w, h, colour_of(name, w, h))
    try:
        for below in BELOWS:
            for levels in LEVELS:
                r.check("%s %dx%d, below %d, %d levels" % (name, w, h, below, levels), below, levels=levels)
    finally:
        r.release()


def test_every_guide_combination(device):
    """all 16 combinations of NULL and given guides at 67 x 35, below = 3 on the mixed set, two levels; no two give the same image"""
    r = Raw(device, 67, 35, colour_of("mixed", 67, 35))
    try:
        seen, pooled = set(), set()
        for mask in range(16):
            seen.add(r.check("guides %s" % format(mask, "04b"), 3, mask, levels=2).tobytes())
            pooled.add(r.check("guides %s, the pool alone" % format(mask, "04b"), 3, mask, levels=0).tobytes())
        assert len(seen) == 16, "two guide combinations gave the same image: a guide is ignored"
        assert len(pooled) == 16, "two guide combinations gave the same pooled variance: the pool ignores a guide"
    finally:
        r.release()


@pytest.mark.parametrize("w,h", [(67, 35), (130, 9)])
def test_both_forms(device, w, h):
    """PT_OPT_DENOISE_SPATIAL_FORM 1 (global gathers), 2 (the LDS tile) and 0 (the shipped choice), each under PT_OPT_DENOISE_TILE 1 and
    2: the same bits"""
    lib = shim.load()
    opt = shim.PT_OPT_DENOISE_SPATIAL_FORM
    assert lib.pt_device_get_option(device._h, opt) == 0
    assert lib.pt_device_set_option(device._h, opt, 3) == E_INV and lib.pt_device_set_option(device._h, opt, -1) == E_INV
    for name, below in (("one_frame", 2), ("mixed", 3), ("synthetic", 2)):
        r = Raw(device, w, h, colour_of(name, w, h))
        try:
            wants = {(levels, mask): r.want(below, mask, levels=levels) for levels, mask in ((0, 15), (2, 15), (5, 15), (1, 0), (1, 4), (1, 2), (1, 9))}
            for form in (1, 2, 0):
                for gather in (1, 2):
                    with options(device, DENOISE_SPATIAL_FORM=form, DENOISE_TILE=gather):
                        assert lib.pt_device_get_option(device._h, opt) == form
                        for (levels, mask), want in wants.items():
                            r.check("%s, form %d, gather %d, %d levels, guides %x" % (name, form, gather, levels, mask), below, mask, want=want, levels=levels)
        finally:
            r.release()


def _short_where(w, h, where):
    """four-sample records everywhere, one sample where `where` holds"""
    rng = np.random.default_rng(5 * w + h)
    s = rng.uniform(0.2, 1.8, (FRAMES, w * h, 3)).astype(F)
    s[1:, where] = np.inf                                                                # rejected: n = 1
    col = mo.accumulate(s)
    assert (col["n"][where] == 1).all() and (col["n"][~where] == FRAMES).all()
    return col


@pytest.mark.parametrize("form", [1, 2])
def test_early_exit(device, form):
    """130 x 9 (five tiles in x, two in y), short pixels only in x < 20: the tiles without one leave before the pool and their pixels
    are pt_denoise's; the first tile column's are the restatement's.  Then 67 x 35 with a single short pixel in a tile's corner, whose
    7 x 7 window spans four tiles of which one alone takes the pass."""
    w, h = 130, 9
    x = np.arange(w * h) % w
    where = (x < 20) & (np.random.default_rng(2).uniform(size=w * h) < 0.5)
    with options(device, DENOISE_SPATIAL_FORM=form):
        r = Raw(device, w, h, _short_where(w, h, where))
        try:
            base = r.plain(params(w, h, levels=0))
            r.reset()
            got = r.check("the pool alone", 2, levels=0)
            far = x >= 32
            assert np.array_equal(got[far], base[far]), "a tile without a short pixel changed"
            # (a pixel whose guides match no neighbour's pools itself alone: 0 again, as the restatement has it)
            assert (got[where, 3] > 0).sum() > where.sum() // 2 and (base[where, 3] == 0).all()
            assert np.array_equal(got[~where], base[~where])
            r.check("five levels", 2, levels=5)
        finally:
            r.release()
        w, h = 67, 35
        where = np.zeros(w * h, bool)
        where[16 * w + 32] = True                                                         # the first pixel of tile (1, 2)
        r = Raw(device, w, h, _short_where(w, h, where))
        try:
            base = r.plain(params(w, h, levels=0))
            r.reset()
            got = r.check("one short pixel, the pool alone", 2, levels=0)
            assert got[where, 3] > 0.5 and np.array_equal(got[~where], base[~where])      # (its neighbours count: the samples lie in 0.2 .. 1.8)
            r.check("one short pixel, five levels", 2, levels=5)
        finally:
            r.release()


@pytest.mark.parametrize("below", [0, 1])
def test_identity_with_pt_denoise(device, below):
    """below 0 and 1 name no pixel: the bits of out are pt_denoise's, on the device"""
    w, h = 67, 35
    r = Raw(device, w, h, colour_of("synthetic", w, h))
    try:
        for levels in LEVELS:
            for mask in (15, 0):
                p = params(w, h, levels=levels)
                base = r.plain(p, mask)
                r.reset()
                assert r.call(p, spatial(below), mask) == shim.PT_OK
                assert r.read()[:w * h].tobytes() == base.tobytes(), (levels, mask)
    finally:
        r.release()


def test_asynchronous_and_allocates_nothing(device):
    """three calls with an event each: the handle's workspace and the device's memory in use stand still, the event completes and
    has measured the call, the versions aside nothing but out and scratch changes"""
    lib = shim.load()
    w, h = 130, 9
    n = w * h
    r = Raw(device, w, h, colour_of("mixed", w, h))
    ev = adl.SyncObject(device)
    try:
        r.check("warm", 3, levels=5)
        ws, used = lib.pt_device_workspace_memory(device._h), lib.pt_device_used_memory(device._h)
        p, sp = params(w, h, levels=5), spatial(3)
        for i in range(3):
            assert r.call(p, sp, ev=ev._h) == shim.PT_OK
            assert lib.pt_device_workspace_memory(device._h) == ws and lib.pt_device_used_memory(device._h) == used
        ev.waitForCompletion()
        assert ev.isComplete() and ev.getExecutionTimeNanoseconds() > 0
        assert_fb_equal(r.read()[:n], r.want(3, levels=5), "after three calls")
        back = np.zeros(n * 56, np.uint8)
        for b, rec in zip(r.bufs, [r.colour] + r.guides):
            b.read(back, n * 56)
            device.waitForCompletion()
            assert back.tobytes() == rec.tobytes(), "an input was written"
    finally:
        ev.release()
        r.release()


def test_argument_errors_leave_out_untouched(device):
    w, h = 5, 4
    r = Raw(device, w, h, colour_of("one_frame", w, h))
    try:
        ok = params(w, h)
        assert r.call(ok, None) == E_INV and b"spatial" in r.lib.pt_last_error()
        assert r.call(ok, spatial(-1)) == E_INV and r.call(ok, spatial(-2 ** 31)) == E_INV
        for k in range(7):
            assert r.call(ok, spatial(2, reserved=k)) == E_INV, k
        # inherited from pt_denoise_params
        assert r.call(None, spatial(2)) == E_INV
        for kw in (dict(levels=9), dict(width=0), dict(reserved=0), dict(reserved=5), dict(sigma_a=float("nan"))):
            assert r.call(params(w, h, **kw), spatial(2)) == E_INV, kw
        assert r.call(params(w + 1, h), spatial(2)) == shim.PT_ERR_RANGE
        sp = spatial(2)
        assert r.lib.pt_denoise_spatial(None, *r.handles(15), ctypes.byref(ok), ctypes.byref(sp), None) == E_INV
        assert r.lib.pt_denoise_spatial(device._h, None, *r.handles(15)[1:], ctypes.byref(ok), ctypes.byref(sp), None) == E_INV
        assert np.array_equal(r.read(), r.sentinel), "an error touched out"
        assert r.call(ok, spatial(2)) == shim.PT_OK
        device.waitForCompletion()
    finally:
        r.release()


# ---- through the renderers -------------------------------------------------------------------------------------------------------
def _records(device, buf, n):
    rec = np.zeros(n, mo.MOMENTS_DTYPE)
    buf.read(rec.view(np.uint8), rec.nbytes)
    device.waitForCompletion()
    return rec


def test_indirect_render_of_one_frame_end_to_end(device, cornell):
    """Cornell 40 x 24, ONE frame: denoiser(spatial_below=2) equals the restatement on the records read back, denoiser() is pt_denoise
    and leaves the image as it found it"""
    from oclpathtracer_amd.denoise import SPATIAL_BELOW
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = cornell
    W, H = 40, 24
    r = IndirectRenderer(device, tris, mats, W, H, max_bounces=4, light_samples=1, moments=True, stripe_rows=1)
    d = f = d0 = None
    try:
        r.render(1)
        d, f = r.denoiser(spatial_below=SPATIAL_BELOW)
        assert d.spatial.below == 2 and f.frames_done == 1
        colour = _records(device, r.mom, W * H)
        assert colour["n"].max() == 1
        guides = [f.moments(name) for name in ("albedo", "normal", "depth", "emission")]
        got = d.denoise(r.mom, f)
        assert_fb_equal(got, dso.denoise(colour, *guides, W, H, 2), "end to end")
        from oclpathtracer_amd.denoise import Denoiser

        d0 = Denoiser(device, W, H)
        assert d0.spatial is None
        plain = d0.denoise(r.mom, f)
        assert_fb_equal(plain, do.denoise(colour, *guides, W, H), "spatial_below = 0 is pt_denoise")
        assert not plain[..., 3].any() and (got[..., 3][colour["n"].reshape(H, W) == 1] > 0).any()
    finally:
        for o in (d, f, d0):
            if o is not None:
                o.release()
        r.release()


def test_temporal_accumulator_after_a_move(device, cornell):
    """render(6), move the eye by 0.3, render(1): the pixels that took no history hold one sample, and the denoiser with
    spatial_below = 2 equals the restatement on the records read back"""
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.denoise import Denoiser
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = cornell
    W, H = 40, 24
    r = IndirectRenderer(device, tris, mats, W, H, max_bounces=4, light_samples=1, moments=True, stripe_rows=1)
    acc = d = None
    try:
        acc = r.temporal()
        acc.render(6)
        acc.move(Camera((0.3, 2.75, 4.0), (0.3, 2.75, 3.0)))
        acc.render(1)
        colour = _records(device, r.mom, W * H)
        short = colour["n"] == 1
        assert short.any() and (colour["n"] > 1).any()
        guides = [acc.features.moments(name) for name in ("albedo", "normal", "depth", "emission")]
        d = Denoiser(device, W, H, spatial_below=2)
        got = d.denoise(r.mom, acc.features)
        assert_fb_equal(got, dso.denoise(colour, *guides, W, H, 2), "after the move")
        assert got.tobytes() != do.denoise(colour, *guides, W, H).tobytes()
    finally:
        for o in (d, acc):
            if o is not None:
                o.release()
        r.release()


# ---- the harness ----------------------------------------------------------------------------------------------------------------
_LINE = re.compile(r"^denoise: levels (\d+) mean_variance unfiltered (\S+) filtered (\S+) spatial below (\d+) pooled_pixels (\d+)\n", re.M)


def test_harness_spatial(device, tmp_path, cornell):
    """raytrace_test --noise --denoise 3 --spatial at 32 x 32, ONE frame: the denoise line gains `below` and the count of pixels that
    took the pooled variance; its two figures are the means of the fourth channel of Denoiser(spatial_below=2)'s output"""
    import os
    import subprocess

    from conftest import ROOT
    from oclpathtracer_amd.indirect import IndirectRenderer

    out, _, _ = harness_ppm(tmp_path, 32, 1, "IndirectIllumination", "--noise", "--denoise", "3", "--spatial")
    assert len(_LINE.findall(out)) == 1
    g = _LINE.search(out).groups()
    tris, mats = cornell
    r = IndirectRenderer(device, tris, mats, 32, 32, max_bounces=16, light_samples=1, stripe_rows=1, chunk_frames=8, moments=True)
    d = f = None
    try:
        r.render(1)
        d, f = r.denoiser(levels=3, spatial_below=2)
        filtered = d.denoise(r.mom, f)[..., 3].astype(np.float64).mean()
        d.params.levels = 0
        unfiltered = d.denoise(r.mom, f)[..., 3].astype(np.float64).mean()
        pooled = int((_records(device, r.mom, 32 * 32)["n"] == 1).sum())
    finally:
        for o in (d, f):
            if o is not None:
                o.release()
        r.release()
    assert int(g[0]) == 3 and int(g[3]) == 2 and int(g[4]) == pooled > 900
    assert abs(float(g[1]) - unfiltered) <= 2e-9 * unfiltered and abs(float(g[2]) - filtered) <= 2e-9 * filtered
    assert 0 < filtered < unfiltered
    # refused without --denoise, as the file's other dependent flags are
    exe = os.path.join(ROOT, "oclpathtracer_amd", "raytrace_test")
    bad = subprocess.run([exe, "--only", "IndirectIllumination", "--noise", "--spatial"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--spatial goes with --denoise" in bad.stderr
