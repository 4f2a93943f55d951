"""pt_sample_moments and pt_moments_resolve on the device, bit for bit against the numpy restatement (tests/moments_oracle.py, which
tests/test_moments_cpu.py checks against exact arithmetic): the raw calls on samples written from the host, the lit renderers'
``moments=True`` against the restatement applied to the oracles' per-sample radiance, the argument errors, and the harness's --noise."""
import re

import numpy as np
import pytest

import indirect_oracle as io
import mis_oracle as mo
import moments_oracle as mom
import power_oracle as po
from conftest import assert_fb_equal
from gpu_support import SEARCHES, harness_ppm, options
from oclpathtracer_amd import adl, scene, shim
from scenes import edge_scene, glossy_room

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE


# ---- the raw calls --------------------------------------------------------------------------------------------------------------
def _random_samples(rng, frames, pixels):
    """float32 [frames, pixels, 3]: decimal exponents -40 .. +38 (subnormals below 1e-38), both signs, +-0, +-FLT_MAX and the smallest
    subnormal sprinkled in, about 5 % of the samples with a NaN or an infinity in ONE channel; with three pixels or more, pixel 1 has
    every sample rejected and the last pixel but one exactly one finite sample."""
    mant = rng.uniform(1.0, 3.4, (frames, pixels, 3)) * rng.choice([-1.0, 1.0], (frames, pixels, 3))
    s = (mant * 10.0 ** rng.integers(-40, 39, (frames, pixels, 3))).astype(np.float32)
    special = np.array([0.0, -0.0, FLT_MAX, -FLT_MAX, 1e-45, -1e-45], np.float32)
    pick = rng.uniform(size=s.shape) < 0.06
    s[pick] = rng.choice(special, int(pick.sum()))
    bad = rng.uniform(size=(frames, pixels)) < 0.05
    if pixels >= 3:
        bad[:, 1] = True
        bad[:, pixels - 2] = True
        bad[frames // 2, pixels - 2] = False
    f, p = np.nonzero(bad)
    s[f, p, rng.integers(0, 3, len(f))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(f))
    assert np.isfinite(s[~bad]).all()
    return s


class _Raw:
    """a sample workspace holding ``s`` and a moments buffer of ``fill`` bytes (or the records ``start``)"""

    def __init__(self, device, s, fill=0xFF, start=None):
        self.device, self.lib = device, shim.load()
        self.frames, self.pixels = s.shape[:2]
        self.sb = adl.Buffer(device, max(s.size, 1), np.float32)
        self.mb = adl.Buffer(device, max(self.pixels, 1) * 56, np.uint8)
        if s.size:
            self.sb.write(np.ascontiguousarray(s), s.size)
        self.before = np.full(max(self.pixels, 1) * 56, fill, np.uint8) if start is None else np.ascontiguousarray(start).view(np.uint8)
        self.mb.write(self.before, self.before.size)

    def accumulate(self, frames, reset, first=0, pixels=None, sb=None, mb=None):
        """pt_sample_moments on frames [first, first + frames) of the workspace (a sub-range wrapped as a buffer of its own)"""
        n = self.pixels if pixels is None else pixels
        if first:
            w = adl.Buffer(dtype=np.float32)
            w.setRawPtr(self.device, self.sb.m_ptr + first * self.pixels * 12, frames * self.pixels * 3)
            try:
                return self.lib.pt_sample_moments(self.device._h, w._h, self.mb._h, n, frames, reset, None)
            finally:
                w.release()
        sb, mb = self.sb if sb is None else sb, self.mb if mb is None else mb
        return self.lib.pt_sample_moments(self.device._h, sb._h if sb != 0 else None, mb._h if mb != 0 else None, n, frames, reset, None)

    def moments(self):
        out = np.zeros(max(self.pixels, 1), mom.MOMENTS_DTYPE)
        self.mb.read(out, out.nbytes)
        self.device.waitForCompletion()
        return out[:self.pixels]

    def assert_untouched(self):
        assert self.moments().tobytes() == self.before[:self.pixels * 56].tobytes(), "the moments were touched"

    def release(self):
        self.sb.release()
        self.mb.release()


def _assert_records_equal(got, want, what):
    for name in mom.MOMENTS_DTYPE.names:
        g, w = got[name], want[name]
        same = g.view(np.uint64) == w.view(np.uint64) if g.dtype == np.float64 else g == w
        assert same.all(), "%s: %s differs at %s (got %r, want %r)" % (what, name, np.argwhere(~same)[:4].tolist(), g[~same][:4], w[~same][:4])


@pytest.mark.parametrize("frames", [1, 2, 7, 8, 9, 64, 65])
@pytest.mark.parametrize("pixels", [1, 63, 64, 65, 255, 257, 1240])
def test_accumulate(device, pixels, frames):
    """partial waves and every remainder of the eight-frame unroll; reset = 1 over a buffer of 0xFF bytes is a start from zeros"""
    s = _random_samples(np.random.default_rng(1000 * pixels + frames), frames, pixels)
    b = _Raw(device, s)
    try:
        assert b.accumulate(frames, 1) == shim.PT_OK
        got, want = b.moments(), mom.accumulate(s)
        _assert_records_equal(got, want, "%d pixels, %d frames" % (pixels, frames))
        if pixels >= 3:
            assert got["n"][1] == 0 and got["rejected"][1] == frames and got["n"][pixels - 2] == 1
        assert int(got["n"].sum()) + int(got["rejected"].sum()) == pixels * frames
    finally:
        b.release()


def test_accumulate_goes_on_from_the_buffer_and_calls_merge(device):
    """reset = 0 starts from the records the buffer holds (counters near 2^32 wrap); calls of 5, 1 and 9 frames equal one of 15"""
    rng = np.random.default_rng(7)
    s = _random_samples(rng, 15, 257)
    start = mom.accumulate(_random_samples(rng, 3, 257))
    start["n"][:8] = 0xFFFFFFFF - np.arange(8, dtype=np.uint32)
    start["rejected"][8:16] = 0xFFFFFFFE
    one, split = _Raw(device, s, start=start), _Raw(device, s)
    try:
        assert one.accumulate(15, 0) == shim.PT_OK
        _assert_records_equal(one.moments(), mom.accumulate(s, start), "from the buffer's records")
        assert split.accumulate(5, 1) == shim.PT_OK and split.accumulate(1, 0, first=5) == shim.PT_OK and split.accumulate(9, 0, first=6) == shim.PT_OK
        _assert_records_equal(split.moments(), mom.accumulate(s), "5 + 1 + 9 frames")
    finally:
        one.release()
        split.release()


def _random_records(rng, pixels):
    """pt_pixel_moments records as a render leaves them and at resolve's edges: n of 0, 1, 2 and up to 2^32 - 1, scales over forty
    decades, sum2 at, just below and just above sum^2 / n (the cancellation: residues of both signs) and well above it"""
    m = mom.zeros(pixels)
    m["n"] = rng.choice(np.array([0, 1, 2, 3, 17, 64, 3200, 0xFFFFFFFF], np.uint32), pixels, p=[.05, .05, .1, .1, .2, .3, .15, .05])
    m["rejected"] = rng.integers(0, 5, pixels)
    n = np.maximum(m["n"].astype(np.float64), 1.0)[:, None]
    mean = rng.normal(size=(pixels, 3)) * 10.0 ** rng.uniform(-20, 20, (pixels, 1))
    m["sum"] = mean * n
    factor = rng.choice([1.0 - 2.0 ** -50, 1.0, 1.0 + 2.0 ** -50, 2.0, 11.0], (pixels, 3)) + rng.choice([0.0, 1.0], (pixels, 3)) * rng.uniform(0, 1, (pixels, 3))
    m["sum2"] = (m["sum"] * m["sum"] / n) * factor
    m["sum"][rng.uniform(size=pixels) < 0.02] = 0.0          # means of 0 with a variance
    return m


_BIG = 2048 * 2048 + 1   # three levels of the tree


# (the 235 MB record buffer of the last size is one case)
@pytest.mark.parametrize("pixels,outputs", [(n, o) for n in (1, 2, 3, 2047, 2048, 2049, 4097) for o in ("noise", "summary", "both")] + [(_BIG, "both")])
def test_resolve(device, pixels, outputs):
    """one tile, its edges, two levels (2 049, 4 097) and three (2 048^2 + 1), with either output and both"""
    lib = shim.load()
    m = _random_records(np.random.default_rng(pixels), pixels)
    assert lib.pt_moments_summary_bytes(pixels) >= 48 and lib.pt_moments_summary_bytes(pixels) % 48 == 0
    mb = adl.Buffer(device, pixels * 56, np.uint8)
    nb = adl.Buffer(device, pixels, adl.float4) if outputs != "summary" else None
    sb = adl.Buffer(device, lib.pt_moments_summary_bytes(pixels), np.uint8) if outputs != "noise" else None
    try:
        mb.write(m.view(np.uint8), m.nbytes)
        assert lib.pt_moments_resolve(device._h, mb._h, pixels, nb._h if nb else None, sb._h if sb else None, None) == shim.PT_OK
        if nb:
            got = np.zeros(pixels, mom.NOISE_DTYPE)
            nb.read(got, got.nbytes // 16)
            device.waitForCompletion()
            want = mom.noise_map(m)
            assert np.array_equal(got["n"], want["n"])
            bad = np.argwhere(got["var"].view(np.uint32) != want["var"].view(np.uint32))
            assert len(bad) == 0, "%d variances differ, first %s: got %r want %r" % (len(bad), bad[0], got["var"][tuple(bad[0])], want["var"][tuple(bad[0])])
            assert not np.signbit(got["var"]).any() and not np.isnan(got["var"]).any()
        if sb:
            got = np.zeros((), mom.SUMMARY_DTYPE)
            sb.read(got.reshape(1), 48)
            device.waitForCompletion()
            want = mom.summary(m)
            assert got.tobytes() == want.tobytes(), "%d pixels: summary %s, want %s" % (pixels, got, want)
            assert int(got["pixels"]) == int((m["n"] >= 2).sum()) > 0 or pixels < 3
    finally:
        for b in (mb, nb, sb):
            if b is not None:
                b.release()


# ---- through the renderers ------------------------------------------------------------------------------------------------------
W, H, FRAMES, CHUNK, K, B = 16, 16, 64, 5, 1, 4
ESTIMATORS = {"plain": dict(), "mis": dict(mis=True), "power": dict(light_choice="power")}
_RAD = {}


def _cornell():
    return edge_scene("cornell")[1][:2]


def _radiance(estimator):
    """float32 [FRAMES, W * H, 3]: the oracle's radiance before the fold of every sample, computed once per estimator"""
    if estimator not in _RAD:
        tris, mats = _cornell()
        if estimator == "power":
            rad = po.radiance_frames(po.INDIRECT, tris, mats, W, H, FRAMES, K, B)
        else:
            rad = mo.radiance_frames(tris, mats, W, H, 0, FRAMES, K, B, mis=estimator == "mis")
        _RAD[estimator] = rad.astype(np.float32)
        _RAD[estimator].setflags(write=False)
    return _RAD[estimator]


def _renderer(device, moments, estimator="plain", **kw):
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = _cornell()
    kw.setdefault("stripe_rows", 1)
    kw.setdefault("chunk_frames", CHUNK)
    return IndirectRenderer(device, tris, mats, W, H, max_bounces=B, light_samples=K, moments=moments, **ESTIMATORS[estimator], **kw)


def _assert_moments_of(r, rad, what):
    """variance() and noise() of renderer ``r`` are the restatement's for the samples ``rad`` [frames, local pixels, 3]"""
    want = mom.accumulate(rad)
    var, n = r.variance()
    wn = mom.noise_map(want)
    assert var.dtype == np.float32 and var.shape == (rad.shape[1], 3) and n.dtype == np.uint32
    assert np.array_equal(n, wn["n"]), what
    assert np.array_equal(var.view(np.uint32), wn["var"].view(np.uint32)), "%s: the variance map differs" % what
    got, fig = r.noise(), mom.noise(want)
    print(what, got)
    assert got == fig and type(got).__name__ == "Noise" and got._fields == fig._fields, "%s: noise() %s, the restatement %s" % (what, got, fig)
    return got


@pytest.mark.parametrize("accel", sorted({a for _, a in SEARCHES}))
@pytest.mark.parametrize("estimator", list(ESTIMATORS))
def test_renderer_moments(device, estimator, accel):
    """64 frames in chunks of 5 (twelve chunks and a remainder of 4): the moments are the restatement's of the oracle's per-sample
    radiance, and the framebuffer is the moments=False render's bit for bit"""
    with options(device, ACCEL=accel):
        r, plain = _renderer(device, True, estimator), _renderer(device, False, estimator)
        try:
            r.render(FRAMES)
            plain.render(FRAMES)
            fig = _assert_moments_of(r, _radiance(estimator), "%s, accel %d" % (estimator, accel))
            assert fig.pixels == W * H and fig.samples == W * H * FRAMES and fig.rejected == 0 and fig.variance_per_sample > 0
            assert_fb_equal(r.read(), plain.read(), "%s, accel %d: the framebuffer with moments" % (estimator, accel))
        finally:
            r.release()
            plain.release()


def test_renderer_moments_on_a_stripe(device):
    """rank 1 of 3 with stripes of one row: the local pixels' moments"""
    r = _renderer(device, True, n_ranks=3, rank=1)
    try:
        r.render(FRAMES)
        rows = [y for y in range(H) if y % 3 == 1]
        assert r.local_pixels == len(rows) * W
        local = _radiance("plain").reshape(FRAMES, H, W, 3)[:, rows].reshape(FRAMES, -1, 3)
        _assert_moments_of(r, local, "rank 1 of 3")
    finally:
        r.release()


def test_glossy_room_counts_its_rejected_samples(device):
    """the glossy room at shift 0 (40 x 24, 3 frames, K = 1, B = 4) makes NaN paths: rejected is the number of the oracle's samples
    with a component that is not finite (tests/test_indirect_cpu.py pins 856 of the 2 880 with a NaN), and nothing is lost"""
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = glossy_room(0)
    gid, frame = io.all_samples(40, 24, 3)
    rad = io.samples(tris, mats, 40, 24, gid, frame, 1, 4)[0].reshape(3, 40 * 24, 3)
    bad = int((~np.isfinite(rad)).any(axis=2).sum())
    r = IndirectRenderer(device, tris, mats, 40, 24, max_bounces=4, light_samples=1, stripe_rows=1, chunk_frames=2, moments=True)
    try:
        r.render(3)
        fig = _assert_moments_of(r, rad, "glossy room")
        print("glossy room: %d of 2880 samples rejected" % fig.rejected)
        assert fig.rejected == bad > 0 and fig.rejected >= 856 and fig.samples + fig.rejected == 2880
    finally:
        r.release()


def test_render_until(device):
    """checks every 8 frames up to 64: with a target between the restatement's figures of two neighbouring checks the render stops at
    the first check below it -- neither the first nor the last --, with a target of 0 at max_frames"""
    rad = _radiance("plain")
    checks = list(range(8, FRAMES + 1, 8))
    rel = [mom.noise(mom.accumulate(rad[:f])).relative_error for f in checks]
    print("relative error at", checks, rel)
    stop = next(i for i in range(2, len(checks) - 1) if rel[i] < min(rel[:i]))   # a check that is the first below its own figure
    target = 0.5 * (rel[stop] + min(rel[:stop]))
    want = next(f for f, e in zip(checks, rel) if e < target)
    assert want == checks[stop] and checks[0] < want < checks[-1]
    r = _renderer(device, True, chunk_frames=8)
    try:
        assert r.render_until(target, FRAMES) == want == r.frames_done
        _assert_moments_of(r, rad[:want], "render_until's stop")
        later = range(want + 3, FRAMES + 1, 3)                               # goes on from frames_done
        again = next((f for f in later if mom.noise(mom.accumulate(rad[:f])).relative_error < target), FRAMES)
        assert r.render_until(target, FRAMES, check_every=3) == again
        r.set_camera(None)
        assert r.render_until(0.0, 21, check_every=4) == 21                  # 4 + 4 + 4 + 4 + 4 + 1
        _assert_moments_of(r, rad[:21], "a target of 0")
        with pytest.raises(ValueError):
            r.render_until(0.5, 30, check_every=0)
    finally:
        r.release()


def test_frame_ranges_camera_and_the_plain_renderer(device):
    rad = _radiance("plain")
    r, plain = _renderer(device, True), _renderer(device, False)
    try:
        r.render(7)
        for begin in (3, 8, 6):
            with pytest.raises(ValueError):
                r.render(2, begin)
        r.render(4, 7)                                   # frames_done
        _assert_moments_of(r, rad[:11], "7 + 4 frames")
        r.render(6, 0)                                   # 0: afresh
        _assert_moments_of(r, rad[:6], "again from frame 0")
        r.set_camera(None)
        assert r.frames_done == 0
        var, n = r.variance()
        assert not var.any() and not n.any() and r.noise()[2:] == (0, 0, 0)
        with pytest.raises(ValueError):
            r.render(2, 6)
        r.render(9)
        _assert_moments_of(r, rad[:9], "after set_camera (the reference's camera again)")
        plain.render(2)
        plain.render(2, 9)                               # no moments: any range, as before
        for call in (plain.variance, plain.noise, lambda: plain.render_until(0.1, 8)):
            with pytest.raises(RuntimeError):
                call()
    finally:
        r.release()
        plain.release()


def test_renderer_passes_moments_through(device):
    from oclpathtracer_amd.render import Renderer

    tris, mats = _cornell()
    base = Renderer(device, tris, mats, W, H, stripe_rows=1)
    d = base.direct_renderer(moments=True, chunk_frames=3)
    i = base.indirect_renderer(moments=True, max_bounces=B, chunk_frames=CHUNK)
    try:
        d.render(7)
        i.render(FRAMES)
        assert d.noise().samples == W * H * 7
        _assert_moments_of(i, _radiance("plain"), "Renderer.indirect_renderer")
    finally:
        d.release()
        i.release()
        base.release()


# ---- argument errors through the raw ABI ----------------------------------------------------------------------------------------
def test_argument_errors_leave_the_moments_untouched(device):
    lib = shim.load()
    s = _random_samples(np.random.default_rng(3), 4, 100)
    b = _Raw(device, s, fill=0xA5)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    ob = adl.Buffer(other, s.size, np.float32)
    big = adl.Buffer(device, 64 * 1024, np.uint8)
    wraps = []

    def wrap(off, nbytes):
        w = adl.Buffer()
        w.setRawPtr(device, big.m_ptr + off, nbytes)
        wraps.append(w)
        return w

    try:
        assert b.accumulate(-1, 1) == E_INV
        assert b.accumulate(4, 1, sb=0) == E_INV and b.accumulate(4, 1, mb=0) == E_INV
        assert lib.pt_sample_moments(None, b.sb._h, b.mb._h, 100, 4, 1, None) == E_INV
        assert b.accumulate(4, 1, sb=ob) == E_INV                                       # a buffer of another device
        assert b.accumulate(5, 1) == E_RANGE and b.accumulate(4, 1, pixels=101) == E_RANGE   # samples, then moments, too small
        assert b.accumulate(0x7FFFFFFF, 1, pixels=0xFFFFFFFF) == E_RANGE                # (the byte count does not wrap)
        assert b.accumulate(4, 1, sb=wrap(2, 4800)) == E_INV                            # samples not 4-byte aligned
        assert b.accumulate(4, 1, sb=wrap(0, 4800), mb=wrap(8196, 5600)) == E_INV        # moments not 8-byte aligned
        assert b.accumulate(4, 1, sb=wrap(0, 4800), mb=wrap(4792, 5600)) == E_INV        # overlap
        assert b.accumulate(4, 1, sb=wrap(0, 4800), mb=wrap(4800, 5600)) == shim.PT_OK   # (adjacent is fine; not b's moments)
        # resolve: its own list
        SB = lib.pt_moments_summary_bytes(100)
        assert SB >= 48 and SB % 8 == 0
        nb, sb = wrap(16384, 1600), wrap(32768, SB)
        res = lambda m, n, no, su: lib.pt_moments_resolve(device._h, m._h if m else None, n, no._h if no else None, su._h if su else None, None)
        assert res(None, 100, nb, sb) == E_INV
        assert res(b.mb, 101, nb, sb) == E_RANGE and res(b.mb, 100, wrap(16384, 1599), sb) == E_RANGE and res(b.mb, 100, nb, wrap(32768, SB - 1)) == E_RANGE
        assert res(b.mb, 100, wrap(16392, 1600), sb) == E_INV                           # noise not 16-byte aligned
        assert res(b.mb, 100, nb, wrap(32772, SB)) == E_INV                             # summary not 8-byte aligned
        assert res(wrap(1004, 5600), 100, nb, sb) == E_INV                              # moments not 8-byte aligned
        assert res(wrap(16384 - 5600 + 8, 5600), 100, nb, sb) == E_INV                  # moments and noise overlap
        assert res(b.mb, 100, nb, wrap(16384 + 1592, SB)) == E_INV                      # noise and summary overlap
        onb = adl.Buffer(other, 1600, np.uint8)
        try:
            assert res(b.mb, 100, onb, sb) == E_INV
        finally:
            onb.release()
        # nothing to do: PT_OK, nothing touched
        assert b.accumulate(0, 1) == shim.PT_OK and b.accumulate(4, 1, pixels=0) == shim.PT_OK
        assert res(b.mb, 0, nb, sb) == shim.PT_OK and res(b.mb, 100, None, None) == shim.PT_OK
        b.assert_untouched()
    finally:
        for w in wraps:
            w.release()
        big.release()
        ob.release()
        b.release()
        adl.DeviceUtils.deallocate(other)


# ---- the harness ----------------------------------------------------------------------------------------------------------------
_NOISE_LINE = re.compile(r"^noise: variance_per_sample (\S+) relative_error (\S+) pixels (\d+) samples (\d+) rejected (\d+)\n", re.M)


@pytest.mark.parametrize("case", ["DirectIllumination", "IndirectIllumination"])
def test_harness_noise(device, tmp_path, case):
    """raytrace_test --noise (32 x 32, 12 frames: its workspace of 8 frames makes a chunk and a remainder) prints the figures noise()
    gives for the same case; without the flag there is no such line and, seconds aside, not a byte of the output differs; both runs
    pass what gpu_support.harness_ppm expects of a run, and their images are the same"""
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.indirect import IndirectRenderer

    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain_out, name, plain_pixels = harness_ppm(tmp_path / "a", 32, 12, case)
    out, noise_name, pixels = harness_ppm(tmp_path / "b", 32, 12, case, "--noise")
    assert name == noise_name and np.array_equal(pixels, plain_pixels)
    assert _NOISE_LINE.search(plain_out) is None and len(_NOISE_LINE.findall(out)) == 1
    mask = lambda t: re.sub(r"in \d+\.\d+ s", "in # s", t).replace(str(tmp_path / "b"), "DIR").replace(str(tmp_path / "a"), "DIR")
    assert mask(_NOISE_LINE.sub("", out)) == mask(plain_out)
    tris, mats = scene.load_model()
    r = DirectRenderer(device, tris, mats, 32, 32, light_samples=4, stripe_rows=1, chunk_frames=8, moments=True) if case == "DirectIllumination" \
        else IndirectRenderer(device, tris, mats, 32, 32, max_bounces=16, light_samples=1, stripe_rows=1, chunk_frames=8, moments=True)
    try:
        r.render(12)
        want = r.noise()
    finally:
        r.release()
    g = _NOISE_LINE.search(out).groups()
    got = (float(g[0]), float(g[1]), int(g[2]), int(g[3]), int(g[4]))
    assert got == tuple(want), (got, want)
