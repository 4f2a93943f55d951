"""pt_denoise on the device, bit for bit -- all four channels -- against the numpy restatement (tests/denoise_oracle.py, which
tests/test_denoise_cpu.py examines on its own): synthetic moments at image sizes that are no multiple of a tile and cross one, every
level count that changes which taps survive, both ends of the normal weight, every combination of guides, both ways a level gathers its
taps, a lit render end to end, the asynchronous call that allocates nothing, the argument errors, and the torch output."""
import ctypes
import re

import numpy as np
import pytest

import denoise_oracle as do
import moments_oracle as mo
from conftest import assert_fb_equal
from gpu_support import harness_ppm, options
from oclpathtracer_amd import adl, shim

pytestmark = pytest.mark.gpu

F = np.float32
E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
FRAMES = 4
SHAPES = [(1, 1), (2, 3), (5, 4), (67, 35), (130, 9)]
LEVELS = [0, 1, 2, 5, 8]
_CASES = {}


def synthetic(w, h):
    """(colour, [albedo, normal, depth, emission]) records of a w x h image, made once per size and shared read-only: three regions --
    a near wall, a far tilted floor and an emitter -- that differ in albedo, normal, depth and emission, a flat patch whose samples
    are all equal (gv = 0 inside it), and sprinkled over them pixels with n = 0 (zero records), only rejected samples, n = 1, never
    hit (no coverage: no depth, zero features) and a zero normal"""
    if (w, h) in _CASES:
        return _CASES[(w, h)]
    rng = np.random.default_rng(1000 * w + h)
    n = w * h
    x, y = np.arange(n) % w, np.arange(n) // w
    region = np.where(x * 3 < w, 0, np.where((y * 2 >= h) & (x * 3 >= 2 * w), 2, 1))
    albedo = np.array([(0.75, 0.25, 0.25), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)], F)[region]
    normal = np.array([(1.0, 0.0, 0.0), (0.0, 0.8, 0.6), (0.0, -1.0, 0.0)], F)[region]
    emit = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (12.0, 9.0, 6.0)], F)[region]
    t = (np.array([2.0, 4.0, 3.0], F)[region] + F(0.03) * x.astype(F) * (region == 1) + F(0.02) * y.astype(F)).astype(F)
    level = np.array([0.4, 1.5, 27.0], F)[region]

    col = (rng.uniform(0.2, 1.8, (FRAMES, n, 3)).astype(F) * level[None, :, None]).astype(F)
    col[:, rng.uniform(size=n) < 0.05] *= F(30.0)                                   # fireflies
    flat = (x >= w // 2) & (x < w // 2 + 6) & (y < 5)
    col[:, flat] = F(0.5)                                                           # equal samples: exact sums, variance 0
    jit = lambda a, s: (a[None] + rng.uniform(-s, s, (FRAMES,) + a.shape)).astype(F)
    alb, nrm, emi = jit(albedo, 0.01), jit(normal, 0.02), np.repeat(emit[None], FRAMES, 0)
    dep = np.zeros((FRAMES, n, 3), F)
    dep[..., 0], dep[..., 1], dep[..., 2] = jit(t, 0.01), 1.0, 0.7
    edge = rng.uniform(size=(FRAMES, n)) < 0.1                                      # partial coverage: a sample that missed
    for a in (alb, nrm, emi, dep):
        a[edge] = 0.0

    pick = lambda p: rng.uniform(size=n) < p
    never, zero_n, rejected, one = pick(0.04), pick(0.04), pick(0.03), pick(0.04)
    for a in (alb, nrm, emi, dep):
        a[:, never] = 0.0
    nrm[:, zero_n] = 0.0
    col[:, rejected] = np.nan
    col[1:, one] = np.inf
    col[0, one] = (0.75, 0.5, 0.25)
    colour = mo.accumulate(col)
    guides = [mo.accumulate(a) for a in (alb, nrm, dep, emi)]
    empty = pick(0.03)
    colour[empty] = 0                                                              # n = 0 and nothing rejected
    guides[1][pick(0.02)] = 0                                                      # a normal record without a sample
    if n > 100:
        assert (colour["n"] == 0).any() and (colour["n"] == 1).any() and (colour["n"] == FRAMES).any() and (colour["rejected"] == FRAMES).any()
        assert (guides[2]["sum"][:, 1] == 0).any() and flat.any() and len(np.unique(region)) == 3
        assert (mo.resolve(colour)[1][flat & (colour["n"] == FRAMES)] == 0).all()
    for a in [colour] + guides:
        a.setflags(write=False)
    _CASES[(w, h)] = (colour, guides)
    return _CASES[(w, h)]


def params(w, h, **kw):
    p = shim.DenoiseParams()
    v = dict(do.DEFAULTS)
    v.update(kw)
    p.width, p.height = w, h
    for k, x in v.items():
        if k == "reserved":
            p.reserved[x] = 1
        else:
            setattr(p, k, x)
    return p


class Raw:
    """The buffers of raw calls of pt_denoise on one synthetic case; `out` starts as a sentinel and has a guard behind it"""

    def __init__(self, device, w, h, pad=3):
        self.device, self.lib, self.w, self.h = device, shim.load(), w, h
        self.colour, self.guides = synthetic(w, h)
        n = w * h
        self.bufs = []
        for rec in [self.colour] + self.guides:
            b = adl.Buffer(device, n * 56, np.uint8)
            b.write(np.ascontiguousarray(rec).view(np.uint8), n * 56)
            self.bufs.append(b)
        self.scratch = adl.Buffer(device, self.lib.pt_denoise_scratch_bytes(w, h), np.uint8)
        self.out = adl.Buffer(device, n + pad, adl.float4)
        self.sentinel = np.full((n + pad, 4), F(-7.25), F)
        self.out.write(self.sentinel, n + pad)

    def call(self, p, mask=15, ev=None, **over):
        """pt_denoise with the guides `mask` names (bit i: guide i of albedo, normal, depth, emission); `over`: colour, g0 .. g3,
        scratch, out replaced (None: a NULL handle)"""
        hs = {"colour": self.bufs[0], "scratch": self.scratch, "out": self.out}
        for i in range(4):
            hs["g%d" % i] = self.bufs[1 + i] if mask >> i & 1 else None
        hs.update(over)
        h = lambda b: b._h if b is not None else None
        return self.lib.pt_denoise(self.device._h, h(hs["colour"]), h(hs["g0"]), h(hs["g1"]), h(hs["g2"]), h(hs["g3"]), h(hs["scratch"]), h(hs["out"]),
                                   ctypes.byref(p) if p is not None else None, ev)

    def read(self):
        got = np.zeros_like(self.sentinel)
        self.out.read(got, len(got))
        self.device.waitForCompletion()
        return got

    def check(self, what, mask=15, **kw):
        """one call under `kw` against the restatement: the image bit for bit, the guard untouched"""
        n = self.w * self.h
        assert self.call(params(self.w, self.h, **kw), mask) == shim.PT_OK, self.lib.pt_last_error()
        got = self.read()
        g = [self.guides[i] if mask >> i & 1 else None for i in range(4)]
        want = do.denoise(self.colour, *g, self.w, self.h, **kw)
        assert_fb_equal(got[:n], want.reshape(n, 4), what)
        assert np.array_equal(got[n:], self.sentinel[n:]), "%s: written behind the image" % what
        return got[:n]

    def release(self):
        for b in self.bufs + [self.scratch, self.out]:
            b.release()


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_parity(device, w, h, levels):
    """every shape at every level count, the normal weight unsquared and squared eight times"""
    r = Raw(device, w, h)
    try:
        for sq in (0, 8):
            r.check("%dx%d, %d levels, %d squarings" % (w, h, levels, sq), levels=levels, normal_squarings=sq)
    finally:
        r.release()


def test_every_guide_combination(device):
    """all 16 combinations of NULL and given guides at 67 x 35, three levels (steps 1, 2 and 4); no two of them give the same image"""
    r = Raw(device, 67, 35)
    try:
        seen = set()
        for mask in range(16):
            got = r.check("guides %s" % format(mask, "04b"), mask, levels=3)
            seen.add(got.tobytes())
        assert len(seen) == 16, "two guide combinations gave the same image: a guide is ignored"
    finally:
        r.release()


@pytest.mark.parametrize("w,h", [(67, 35), (130, 9)])
def test_both_gathers(device, w, h):
    """PT_OPT_DENOISE_TILE 1 (global gathers), 2 (the LDS halo tile at steps 1 and 2) and 0 (the shipped choice): the same bits"""
    lib = shim.load()
    assert lib.pt_device_get_option(device._h, shim.PT_OPT_DENOISE_TILE) == 0
    assert lib.pt_device_set_option(device._h, shim.PT_OPT_DENOISE_TILE, 3) == E_INV and lib.pt_device_set_option(device._h, shim.PT_OPT_DENOISE_TILE, -1) == E_INV
    r = Raw(device, w, h)
    try:
        for mode in (1, 2, 0):
            with options(device, DENOISE_TILE=mode):
                assert lib.pt_device_get_option(device._h, shim.PT_OPT_DENOISE_TILE) == mode
                for levels, mask in ((1, 15), (2, 15), (5, 15), (2, 0), (2, 4), (2, 2)):
                    r.check("gather %d, %d levels, guides %x" % (mode, levels, mask), mask, levels=levels)
    finally:
        r.release()


def test_other_parameters(device):
    """sigmas and eps far from the defaults, among them ones that make a weight underflow and ones that switch a term off"""
    r = Raw(device, 67, 35)
    try:
        r.check("tight", levels=3, sigma_l=0.05, sigma_z=0.01, sigma_a=1e-6, sigma_e=1e-6, eps_l=1e-30, eps_z=1e-30, normal_squarings=3)
        r.check("loose", levels=4, sigma_l=1e6, sigma_z=1e6, sigma_a=1e6, sigma_e=1e6, eps_l=10.0, eps_z=10.0, normal_squarings=1)
    finally:
        r.release()


def test_asynchronous_and_allocates_nothing(device):
    """three calls with an event each: the handle's workspace and the device's memory in use stand still, the event completes and
    has measured the call, the versions aside nothing but out and scratch changes"""
    lib = shim.load()
    r = Raw(device, 130, 9)
    ev = adl.SyncObject(device)
    try:
        r.check("warm", levels=5)
        ws, used = lib.pt_device_workspace_memory(device._h), lib.pt_device_used_memory(device._h)
        p = params(130, 9, levels=5)
        for i in range(3):
            assert r.call(p, ev=ev._h) == shim.PT_OK
            assert lib.pt_device_workspace_memory(device._h) == ws and lib.pt_device_used_memory(device._h) == used
        ev.waitForCompletion()
        assert ev.isComplete() and ev.getExecutionTimeNanoseconds() > 0
        n = 130 * 9
        assert_fb_equal(r.read()[:n], do.denoise(r.colour, *r.guides, 130, 9, levels=5).reshape(n, 4), "after three calls")
        back = np.zeros(n * 56, np.uint8)
        for b, rec in zip(r.bufs, [r.colour] + r.guides):
            b.read(back, n * 56)
            device.waitForCompletion()
            assert back.tobytes() == rec.tobytes(), "an input was written"
    finally:
        ev.release()
        r.release()


def test_argument_errors_leave_out_untouched(device):
    lib = shim.load()
    w, h = 5, 4
    n = w * h
    r = Raw(device, w, h)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    ob = adl.Buffer(other, n * 56, np.uint8)
    big = adl.Buffer(device, 64 * 1024, np.uint8)
    SB = lib.pt_denoise_scratch_bytes(w, h)
    wraps = []

    def wrap(off, nbytes):
        b = adl.Buffer()
        b.setRawPtr(device, big.m_ptr + off, nbytes)
        wraps.append(b)
        return b

    try:
        ok = params(w, h)
        assert lib.pt_denoise(None, r.bufs[0]._h, None, None, None, None, r.scratch._h, r.out._h, ctypes.byref(ok), None) == E_INV
        assert r.call(None) == E_INV
        for name in ("colour", "scratch", "out"):
            assert r.call(ok, **{name: None}) == E_INV, name
        for name in ("colour", "g0", "g1", "g2", "g3", "scratch", "out"):
            assert r.call(ok, **{name: ob}) == E_INV, name                                # a buffer of another device
        for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(width=65536, height=32768), dict(levels=-1), dict(levels=9),
                   dict(normal_squarings=-1), dict(normal_squarings=9), dict(reserved=0), dict(reserved=5)):
            assert r.call(params(w, h, **kw)) == E_INV, kw
        for name in ("sigma_l", "sigma_z", "sigma_a", "sigma_e", "eps_l", "eps_z"):
            for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), 1e-50):              # (1e-50 is 0 in binary32)
                assert r.call(params(w, h, **{name: bad})) == E_INV, (name, bad)
        # too small: RANGE
        assert r.call(params(w + 1, h)) == E_RANGE
        for name in ("colour", "g0", "g1", "g2", "g3"):
            assert r.call(ok, **{name: wrap(0, n * 56 - 1)}) == E_RANGE, name
        assert r.call(ok, out=wrap(0, n * 16 - 1)) == E_RANGE and r.call(ok, scratch=wrap(0, SB - 1)) == E_RANGE
        # alignment
        for name in ("colour", "g0", "g1", "g2", "g3"):
            assert r.call(ok, **{name: wrap(4, n * 56)}) == E_INV, name
        assert r.call(ok, out=wrap(8, n * 16)) == E_INV and r.call(ok, scratch=wrap(8, SB)) == E_INV
        # overlap: of an input with an output, of the two outputs, of two inputs
        assert r.call(ok, colour=wrap(0, n * 56), out=wrap(n * 56 - 16 - (n * 56 - 16) % 16, n * 16)) == E_INV
        assert r.call(ok, out=wrap(16384, n * 16), scratch=wrap(16384 + n * 16 - 16, SB)) == E_INV
        assert r.call(ok, g1=wrap(32768, n * 56), scratch=wrap(32768 - SB + 16, SB)) == E_INV
        assert r.call(ok, g0=r.bufs[3]) == E_INV
        assert np.array_equal(r.read(), r.sentinel), "an error touched out"
        # (adjacent ranges are fine)
        assert r.call(ok, colour=wrap(0, n * 56), out=r.out, scratch=wrap(32768, SB)) == shim.PT_OK
        device.waitForCompletion()
    finally:
        for b in wraps:
            b.release()
        big.release()
        ob.release()
        r.release()
        adl.DeviceUtils.deallocate(other)


# ---- through the renderers -------------------------------------------------------------------------------------------------------
def test_indirect_render_end_to_end(device, cornell):
    """Cornell 48 x 40, 8 frames, MIS with the light chosen by power: denoiser() brings a feature renderer to the renderer's frames,
    and the output is the restatement applied to the moments read back from the device; torch's output is the same"""
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = cornell
    W, H = 48, 40
    r = IndirectRenderer(device, tris, mats, W, H, mis=True, light_choice="power", moments=True, stripe_rows=1)
    d = f = None
    try:
        r.render(8)
        d, f = r.denoiser()
        assert f.frames_done == 8 and f.features == ("albedo", "normal", "depth", "emission")
        got = d.denoise(r.mom, f)
        assert got.shape == (H, W, 4) and got.dtype == np.float32
        colour = np.zeros(W * H, mo.MOMENTS_DTYPE)
        r.mom.read(colour.view(np.uint8), colour.nbytes)
        device.waitForCompletion()
        guides = [f.moments(name) for name in ("albedo", "normal", "depth", "emission")]
        assert colour["n"].max() == 8 and (guides[2]["sum"][:, 1] > 0).any()
        want = do.denoise(colour, *guides, W, H)
        assert_fb_equal(got, want, "end to end")
        noisy = do.denoise(colour, *guides, W, H, levels=0)
        # (a weighted mean of a pixel's neighbours, not a bound per pixel: over the image the variance left must be less than it was)
        assert got[..., 3].mean() < noisy[..., 3].mean(), "the filter left more variance than it found"
        torch = pytest.importorskip("torch")
        t = d.denoise(r.mom, f, as_tensor=True)
        torch.cuda.synchronize()
        assert t.shape == (H, W, 4) and t.dtype == torch.float32
        assert_fb_equal(t.cpu().numpy(), want, "as_tensor")
        # render on: both by the same frames, and the filter follows
        r.render(3)
        f.render(3)
        r.mom.read(colour.view(np.uint8), colour.nbytes)
        device.waitForCompletion()
        guides = [f.moments(name) for name in ("albedo", "normal", "depth", "emission")]
        assert_fb_equal(d.denoise(r.mom, f), do.denoise(colour, *guides, W, H), "after three more frames")
        assert_fb_equal(d.denoise(r.mom), do.denoise(colour, None, None, None, None, W, H), "without features")
        with pytest.raises(ValueError):
            DirectRenderer(device, tris, mats, W, H, stripe_rows=1).denoiser()
        two = DirectRenderer(device, tris, mats, W, H, stripe_rows=8, n_ranks=2, rank=0, moments=True)
        try:
            with pytest.raises(ValueError):
                two.denoiser()
        finally:
            two.release()
    finally:
        for o in (d, f):
            if o is not None:
                o.release()
        r.release()


def test_direct_renderer_with_kept_features(device, cornell):
    """DirectRenderer.denoiser(levels=2) and a feature renderer of the caller's that keeps normal and depth only: the other two guides
    are left out of the call"""
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.features import FeatureRenderer

    tris, mats = cornell
    W, H = 33, 17
    r = DirectRenderer(device, tris, mats, W, H, light_samples=2, moments=True, stripe_rows=1)
    d = f = f2 = None
    try:
        r.render(5)
        d, f = r.denoiser(levels=2, sigma_l=2.0)
        f2 = FeatureRenderer(device, tris, mats, W, H, features=("depth", "normal"), stripe_rows=1)
        with pytest.raises(ValueError):
            d.denoise(r.mom, f2)                       # nothing rendered yet
        f2.render(5)
        colour = np.zeros(W * H, mo.MOMENTS_DTYPE)
        r.mom.read(colour.view(np.uint8), colour.nbytes)
        device.waitForCompletion()
        want = do.denoise(colour, None, f2.moments("normal"), f2.moments("depth"), None, W, H, levels=2, sigma_l=2.0)
        assert_fb_equal(d.denoise(r.mom, f2), want, "normal and depth only")
        assert_fb_equal(d.denoise(r.mom, f), do.denoise(colour, *[f.moments(n) for n in ("albedo", "normal", "depth", "emission")], W, H,
                                                        levels=2, sigma_l=2.0), "all four")
    finally:
        for o in (d, f, f2):
            if o is not None:
                o.release()
        r.release()


# ---- the harness ----------------------------------------------------------------------------------------------------------------
_DENOISE_LINE = re.compile(r"^denoise: levels (\d+) mean_variance unfiltered (\S+) filtered (\S+)\n", re.M)


def test_harness_denoise(device, tmp_path, cornell):
    """raytrace_test --noise --denoise 3 (32 x 32, 12 frames) prints one line more than --noise alone and changes nothing else; its two
    figures are the means of the fourth channel of Denoiser's output at 0 and 3 levels for the same render"""
    from oclpathtracer_amd.indirect import IndirectRenderer

    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain_out, name, plain_pixels = harness_ppm(tmp_path / "a", 32, 12, "IndirectIllumination", "--noise")
    out, dn_name, pixels = harness_ppm(tmp_path / "b", 32, 12, "IndirectIllumination", "--noise", "--denoise", "3")
    assert name == dn_name and np.array_equal(pixels, plain_pixels)
    assert _DENOISE_LINE.search(plain_out) is None and len(_DENOISE_LINE.findall(out)) == 1
    mask = lambda t: re.sub(r"in \d+\.\d+ s", "in # s", t).replace(str(tmp_path / "b"), "DIR").replace(str(tmp_path / "a"), "DIR")
    assert mask(_DENOISE_LINE.sub("", out)) == mask(plain_out)
    tris, mats = cornell
    r = IndirectRenderer(device, tris, mats, 32, 32, max_bounces=16, light_samples=1, stripe_rows=1, chunk_frames=8, moments=True)
    d = f = None
    try:
        r.render(12)
        d, f = r.denoiser(levels=3)
        filtered = d.denoise(r.mom, f)[..., 3].astype(np.float64).mean()
        d.params.levels = 0
        unfiltered = d.denoise(r.mom, f)[..., 3].astype(np.float64).mean()
    finally:
        for o in (d, f):
            if o is not None:
                o.release()
        r.release()
    g = _DENOISE_LINE.search(out).groups()
    assert int(g[0]) == 3
    # (the harness sums the 1 024 floats in a double from first to last, numpy pairwise; it prints nine digits)
    assert abs(float(g[1]) - unfiltered) <= 2e-9 * unfiltered and abs(float(g[2]) - filtered) <= 2e-9 * filtered
    assert 0 < filtered < unfiltered
