"""pt_radiance_rays on the device (include/pt_shim.h states the contract): the workspace and the moments bit for bit against the CPU
restatement (tests/rays_oracle.py) for the four estimators under every search, at the ray counts where the refilling kernels change
their shape, at the ends of the id and sample ranges; the LBVH against brute force with far origins; against the device's own ray
queries; the chunk loop; calls that enqueue nothing; every argument error; the deferred traversal error; RadianceCaster."""
import ctypes

import numpy as np
import pytest

import moments_oracle
import rays_oracle
import scenes
from conftest import assert_fb_equal
from gpu_support import SEARCHES, assert_cut_short_search_is_reported, cornell_rays, options
from oclpathtracer_amd import adl, radiance, scene, shim
from oclpathtracer_amd.direct import light_counts, light_table
from oclpathtracer_amd.indirect import IndirectRenderer, Roulette
from oclpathtracer_amd.query import RayCaster

pytestmark = pytest.mark.gpu

ESTIMATORS = [(False, False), (True, False), (False, True), (True, True)]   # (mis, power)
COUNTS = (1, 63, 65, 257, 1031)   # a lane, a wave short of one, a wave and one, one PT_RR_RUN run and one, workgroups and a partial wave
NMAX, K, B, RR = 1031, 2, 4, (2, 0.9)
TOP = 0x7fffffff
SENTINEL = 0xA5


class Raw:
    """The buffers of raw pt_radiance_rays calls on one scene: the scene, the list, its counts and table, the rays, a workspace and
    moments that start as sentinel bytes (with ``pad`` bytes more than a call may touch)."""

    def __init__(self, device, tris, mats, lights, nmax=NMAX, smax=8):
        self.device, self.lib = device, shim.load()
        self.ntri, self.nmat, self.lights = len(tris), len(mats), np.asarray(lights, np.int32)
        self.tb = adl.Buffer(device, max(len(tris), 1), scene.TRIANGLE_DTYPE)
        self.mb = adl.Buffer(device, len(mats), scene.MATERIAL_DTYPE)
        self.lb = adl.Buffer(device, max(len(self.lights), 1), np.int32)
        if len(tris):
            self.tb.write(tris, len(tris))
        self.mb.write(mats, len(mats))
        if len(self.lights):
            self.lb.write(self.lights, len(self.lights))
        if len(self.lights):
            self.cb = light_counts(self.lib, device, self.lb._h, len(self.lights), self.ntri)
            self.cdf, self.triq = light_table(self.lib, device, self.tb, self.ntri, self.mb, self.nmat, self.lb._h, len(self.lights))
        else:   # (no list: neither is read)
            self.cb, self.triq = adl.Buffer(device, max(self.ntri, 1), np.int32), adl.Buffer(device, max(self.ntri, 1), np.uint32)
            self.cdf = adl.Buffer(device, 4, np.uint64)
        self.rb = adl.Buffer(device, 32 * nmax, np.uint8)
        self.sb = adl.Buffer(device, 12 * nmax * smax + 64, np.uint8)
        self.qb = adl.Buffer(device, 56 * nmax + 64, np.uint8)
        self.fill()

    def fill(self):
        for b in (self.sb, self.qb):
            b.write(np.full(b.getSize(), SENTINEL, np.uint8), b.getSize())

    def params(self, n, count, *, begin=0, first=0, reset=1, nl=None, **kw):
        p = shim.RadianceParams()
        p.num_rays, p.first_ray, p.sample_begin, p.sample_count = n, first, begin, count
        p.num_triangles, p.num_materials, p.num_lights = self.ntri, self.nmat, len(self.lights) if nl is None else nl
        p.light_samples, p.max_bounces, p.reset = K, B, reset
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    def call(self, p, mis=False, power=False, rr=RR, **over):
        """the entry point on these buffers, each replaced by what ``over`` names for it (None: a NULL handle)"""
        h = {}
        for name in ("tb", "mb", "lb", "cb", "cdf", "triq", "rb", "sb", "qb"):
            b = over.get(name, getattr(self, name))
            h[name] = b._h if b is not None else None
        if not len(self.lights) and "lb" not in over:
            h["lb"] = None
        if not power and "cdf" not in over and "triq" not in over:
            h["cdf"] = h["triq"] = None
        if not mis and "cb" not in over:
            h["cb"] = None
        r = shim.Roulette(rr[0], rr[1]) if rr is not None else None
        return self.lib.pt_radiance_rays(self.device._h, h["tb"], h["mb"], h["lb"], int(mis), h["cb"], h["cdf"], h["triq"], h["rb"], h["sb"],
                                         h["qb"], ctypes.byref(p) if p is not None else None, ctypes.byref(r) if r is not None else None, None)

    def run(self, R, count, *, mis=False, power=False, rr=RR, **kw):
        """one call over the rays R that must succeed: (the first ``count`` samples of the workspace [count, n, 3], the moments [n])"""
        r8 = rays_oracle.records(R)
        n = len(r8)
        if n:
            self.rb.write(r8.view(np.uint8).reshape(-1), r8.nbytes)
        rc = self.call(self.params(n, count, **kw), mis, power, rr)
        assert rc == shim.PT_OK, (rc, self.lib.pt_last_error())
        return self.workspace(count, n), self.moments(n)

    def workspace(self, count, n):
        ws = np.zeros((count, n, 3), np.float32)
        if ws.size:
            self.sb.read(ws.view(np.uint8).reshape(-1), ws.nbytes)
        self.device.waitForCompletion()
        return ws

    def moments(self, n):
        m = np.zeros(n, moments_oracle.MOMENTS_DTYPE)
        if n:
            self.qb.read(m.view(np.uint8).reshape(-1), m.nbytes)
        self.device.waitForCompletion()
        return m

    def assert_untouched(self, what=""):
        for b in (self.sb, self.qb):
            got = np.zeros(b.getSize(), np.uint8)
            b.read(got, b.getSize())
            self.device.waitForCompletion()
            assert np.all(got == SENTINEL), "%s: a buffer was touched" % what

    def release(self):
        for b in (self.tb, self.mb, self.lb, self.cb, self.cdf, self.triq, self.rb, self.sb, self.qb):
            b.release()


def assert_moments_equal(got, want, what):
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["rejected"], want["rejected"]), what + ": counts"
    assert_fb_equal(got["sum"].view(np.float32), want["sum"].view(np.float32), what + ": sums")
    assert_fb_equal(got["sum2"].view(np.float32), want["sum2"].view(np.float32), what + ": sums of squares")


def _check(raw, R, want, count, what, **kw):
    raw.fill()
    ws, mom = raw.run(R, count, **kw)
    assert_fb_equal(ws, want, what)
    assert_moments_equal(mom, rays_oracle.moments(want), what)
    pad = np.zeros(64, np.uint8)   # nothing is written behind what the call owns
    raw.sb.read(pad, 64, 12 * len(R) * count)
    raw.device.waitForCompletion()
    assert np.all(pad == SENTINEL), what + ": written past the samples"


_REF = {}


def _cornell_case(cornell, mis, power):
    """(rays, the restatement's workspaces) on the Cornell box, once per estimator: 2 samples from 0 of ids from 0; 2 samples from 5 of
    ids from 1 000; 2 samples that end at 2^31 - 1 of ids that end at 2^31 - 1.  A sample is its id and its number: the first n rays'
    workspace is a slice"""
    key = (mis, power)
    if key not in _REF:
        tris, mats = cornell
        R = _REF.setdefault("rays", cornell_rays(np.random.default_rng(3), NMAX, tris))
        lights = scene.emitters(tris, mats)
        kw = dict(mis=mis, power=power, lights=lights)
        _REF[key] = {(f, s): rays_oracle.workspace(tris, mats, R, 2, K, B, RR, first_ray=f, sample_begin=s, **kw)
                     for f, s in ((0, 0), (1000, 5), (TOP - NMAX, TOP - 2))}
    return _REF["rays"], _REF[key]


@pytest.fixture(scope="module")
def raw_cornell(device, cornell):
    tris, mats = cornell
    r = Raw(device, tris, mats, scene.emitters(tris, mats))
    yield r
    r.release()


@pytest.mark.parametrize("quad,accel", SEARCHES)
@pytest.mark.parametrize("mis,power", ESTIMATORS)
def test_workspace_and_moments_equal_the_restatement(device, cornell, raw_cornell, mis, power, quad, accel):
    R, ref = _cornell_case(cornell, mis, power)
    spread = np.unique(ref[(0, 0)].reshape(-1, 3), axis=0).shape[0]
    assert spread > NMAX // 2, "the restatement's samples hardly differ: %d values" % spread
    with options(device, QUAD_FILTER=quad, ACCEL=accel):
        for n in COUNTS:
            for first, begin in ((0, 0), (1000, 5)):
                _check(raw_cornell, R[:n], ref[(first, begin)][:, :n], 2, "n %d from id %d, sample %d" % (n, first, begin),
                       mis=mis, power=power, first=first, begin=begin)
        # the ends of both ranges: ids and sample numbers up to 2^31 - 2
        for n in (65, NMAX):
            _check(raw_cornell, R[NMAX - n:], ref[(TOP - NMAX, TOP - 2)][:, NMAX - n:], 2, "the last %d ids, the last samples" % n,
                   mis=mis, power=power, first=TOP - n, begin=TOP - 2)


@pytest.mark.parametrize("mis,power", ESTIMATORS)
def test_tiled_table(device, mis, power):
    """more than 256 triangles under brute force: the tiled table's forms"""
    tris, mats = scenes.nested_boxes(8)
    assert len(tris) > 256
    lights = scene.emitters(tris, mats)
    R = cornell_rays(np.random.default_rng(8), 257, tris)
    want = rays_oracle.workspace(tris, mats, R, 2, K, B, RR, first_ray=3, sample_begin=1, mis=mis, power=power, lights=lights)
    raw = Raw(device, tris, mats, lights, nmax=257)
    try:
        for quad in (0, 4):
            with options(device, QUAD_FILTER=quad, ACCEL=1):
                _check(raw, R, want, 2, "tiled, filter %d" % quad, mis=mis, power=power, first=3, begin=1)
    finally:
        raw.release()


@pytest.mark.parametrize("name,accel,form", [("slab:1", 1, "lds"), ("slab:10", 1, "tiled"), ("slab:15", 0, "lbvh")])
def test_unbounded_forms(device, name, accel, form):
    """one huge triangle lifts the scene over PT_DET_BOUND_MAX: the DET_BOUNDED = false instantiations, on a scene they can shade"""
    import lit_cells

    tris, mats, lights, _ = scenes.edge_scene(name)[1]
    assert lit_cells.form_of(tris, 0, accel) == (form, False, 0)
    R = cornell_rays(np.random.default_rng(10), 257, tris[:36])   # (the first box: rays about it, not about the slab)
    raw = Raw(device, tris, mats, lights, nmax=257)
    try:
        with options(device, QUAD_FILTER=0, ACCEL=accel):
            for mis, power in ESTIMATORS:
                want = rays_oracle.workspace(tris, mats, R, 2, K, B, RR, first_ray=9, sample_begin=3, mis=mis, power=power, lights=lights)
                assert (want != np.float32(0.45)).any(axis=2).mean() > 0.3, "hardly a ray is shaded"
                _check(raw, R, want, 2, "%s, mis %d power %d" % (form, mis, power), mis=mis, power=power, first=9, begin=3)
    finally:
        raw.release()


@pytest.mark.parametrize("accel", (1, 2))
def test_glossy_room_mis(device, accel):
    """MIS where it matters: GGX surfaces next to the light, every roughness that keeps a path finite"""
    tris, mats = scenes.glossy_room(5, scenes.FINITE_ROUGHNESS)
    lights = scene.emitters(tris, mats)
    R = cornell_rays(np.random.default_rng(9), 300, tris)
    raw = Raw(device, tris, mats, lights, nmax=300)
    try:
        for power in (False, True):
            want = rays_oracle.workspace(tris, mats, R, 3, K, 6, (3, 0.95), mis=True, power=power, lights=lights)
            with options(device, ACCEL=accel):
                r8 = rays_oracle.records(R)
                raw.rb.write(r8.view(np.uint8).reshape(-1), r8.nbytes)
                assert raw.call(raw.params(300, 3, max_bounces=6), True, power, (3, 0.95)) == shim.PT_OK
                assert_fb_equal(raw.workspace(3, 300), want, "glossy room, power %d" % power)
                assert_moments_equal(raw.moments(300), rays_oracle.moments(want), "glossy room, power %d" % power)
    finally:
        raw.release()


def _soup_rays(tris, n, seed):
    """rays through the soup, a third of them from 100 scene sizes away, aimed back at it"""
    rng = np.random.default_rng(seed)
    R = np.zeros((n, 8), np.float32)
    R[:, :3] = rng.uniform(-3.5, 3.5, (n, 3))
    R[:, 3] = 1e20
    R[:, 4:7] = rng.normal(size=(n, 3))
    far = np.arange(n) % 3 == 0
    target = rng.uniform(-2.5, 2.5, (n, 3)).astype(np.float32)
    R[far, :3] = (rng.normal(size=(n, 3)) * 600.0 / np.sqrt(3.0)).astype(np.float32)[far]
    R[far, 4:7] = (target - R[:, :3])[far]
    return R


def test_lbvh_equals_brute_force(device):
    tris = scenes.soup(2000)
    mats = np.zeros(7, scene.MATERIAL_DTYPE)
    mats["albedo"][:, :3] = np.linspace(0.2, 0.8, 21, dtype=np.float32).reshape(7, 3)
    mats["emissive"][5, :3] = (4.0, 3.0, 2.0)
    lights = scene.emitters(tris, mats)
    assert 100 < len(lights) < 1000
    R = _soup_rays(tris, 1031, 17)
    assert np.abs(R[::3, :3]).max() > 300.0
    raw = Raw(device, tris, mats, lights)
    try:
        for mis, power in ESTIMATORS:
            got = {}
            for accel in (1, 2):
                with options(device, ACCEL=accel):
                    got[accel] = raw.run(R, 2, mis=mis, power=power, begin=4, first=11)
            assert_fb_equal(got[2][0], got[1][0], "LBVH against brute force, mis %d power %d" % (mis, power))
            assert_moments_equal(got[2][1], got[1][1], "LBVH against brute force")
            hit = got[1][0][0] != np.float32(0.45)
            assert hit.any(axis=1)[::3].sum() > 30, "hardly a far ray reaches the soup"
    finally:
        raw.release()


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_one_vertex_is_the_emission_at_the_query_hit(device, cornell, quad, accel):
    """the device alone: B = 1, no lights -- 3 x emissive at pt_intersect_rays' hit of the same rays, 0.45 on its misses; tmax is not read"""
    tris, mats = cornell
    R = cornell_rays(np.random.default_rng(12), 1031, tris)
    lamp = scene.emitters(tris, mats)
    R[:60, 4:7] = (tris["p1"][lamp[0], :3] + tris["p2"][lamp[0], :3] + tris["p3"][lamp[0], :3]) / np.float32(3.0) - R[:60, :3]
    R[100:110, 4:7] = 0.0                                  # zero-length directions
    R[110:120, 5] = np.nan                                 # NaN directions
    R[120:125, 4] = np.inf
    Q = R.copy()                                           # what the query sees: every ray unbounded
    R[0::5, 3], R[1::5, 3], R[2::5, 3] = 0.0, np.nan, 1e-3
    R[:, 7] = np.arange(len(R), dtype=np.int32).view(np.float32)
    raw = Raw(device, tris, mats, [])
    caster = RayCaster(device, tris)
    try:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            hit = caster.closest(Q)
            ws, mom = raw.run(R, 1, max_bounces=1, first=7, begin=2)
        want = np.full((len(R), 3), np.float32(0.45), np.float32)
        on = hit["tri"] >= 0
        want[on] = np.maximum(np.float32(0.0) + np.float32(1.0) * mats["emissive"][hit["material"][on], :3] * np.float32(3.0), np.float32(0.0))
        assert on.sum() > 400 and (~on).sum() > 100 and (want[:60].max(axis=1) > 0.45).sum() >= 10
        assert_fb_equal(ws[0], want, "emission at the query's hit")
        assert np.array_equal(mom["n"] + mom["rejected"], np.ones(len(R), np.uint32))
    finally:
        caster.release()
        raw.release()


def test_chunks_calls_and_ray_ranges_compose(device, cornell, raw_cornell):
    tris, mats = cornell
    raw = raw_cornell
    R, _ = _cornell_case(cornell, True, True)
    kw = dict(mis=True, power=True)
    ws7, mom7 = raw.run(R, 7, first=40, begin=9, **kw)                      # the whole call in one chunk
    want = rays_oracle.workspace(tris, mats, R[:65], 7, K, B, RR, first_ray=40, sample_begin=9, lights=scene.emitters(tris, mats), **kw)
    assert_fb_equal(ws7[:, :65], want, "seven samples")
    # a workspace of three samples: chunks of 3, 3 and 1
    small = adl.Buffer(device, 12 * NMAX * 3 + 11, np.uint8)
    try:
        raw.fill()
        r8 = rays_oracle.records(R)
        raw.rb.write(r8.view(np.uint8).reshape(-1), r8.nbytes)
        assert raw.call(raw.params(NMAX, 7, first=40, begin=9), sb=small, **kw) == shim.PT_OK
        assert_moments_equal(raw.moments(NMAX), mom7, "chunks of 3, 3, 1")
        last = np.zeros((NMAX, 3), np.float32)
        small.read(last.view(np.uint8).reshape(-1), last.nbytes)
        device.waitForCompletion()
        assert_fb_equal(last, ws7[6], "the last chunk's sample")
        # without moments nothing consumes a chunk: the workspace must hold the call
        assert raw.call(raw.params(NMAX, 7), sb=small, qb=None, **kw) == shim.PT_ERR_RANGE
        assert raw.call(raw.params(NMAX, 3), sb=small, qb=None, **kw) == shim.PT_OK
    finally:
        small.release()
    # two calls of 3 and 4 samples, reset then not
    raw.fill()
    raw.run(R, 3, first=40, begin=9, reset=1, **kw)
    ws4, mom = raw.run(R, 4, first=40, begin=12, reset=0, **kw)
    assert_moments_equal(mom, mom7, "3 + 4 samples")
    assert_fb_equal(ws4, ws7[3:], "the later samples")
    # two ray ranges with matching ids
    a, ma = raw.run(R[:500], 7, first=40, begin=9, **kw)
    b, mb = raw.run(R[500:], 7, first=540, begin=9, **kw)
    assert_fb_equal(np.concatenate([a, b], axis=1), ws7, "rays [0, 500) and [500, 1031)")
    assert_moments_equal(np.concatenate([ma, mb]), mom7, "rays [0, 500) and [500, 1031)")


def test_nothing_is_enqueued_for_no_rays_or_no_samples(device, cornell, raw_cornell):
    raw = raw_cornell
    raw.fill()
    for n, count in ((0, 4), (5, 0), (0, 0)):
        for reset in (0, 1):
            assert raw.call(raw.params(n, count, reset=reset), True, True) == shim.PT_OK, (n, count)
            assert raw.call(raw.params(n, count, reset=reset), qb=None) == shim.PT_OK, (n, count)
    raw.assert_untouched("no rays or no samples")


def test_an_empty_scene_is_the_background(device, cornell):
    tris, mats = cornell
    raw = Raw(device, tris[:0], mats, [], nmax=70)
    try:
        ws, mom = raw.run(cornell_rays(np.random.default_rng(2), 70, tris), 2)
        assert np.all(ws == np.float32(0.45)) and np.all(mom["n"] == 2)
    finally:
        raw.release()


def test_argument_errors_leave_the_buffers_untouched(device, cornell, raw_cornell):
    raw = raw_cornell
    raw.fill()
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    n = 100
    est = dict(mis=True, power=True)
    cases = [(dict(begin=-1), E_INV), (dict(sample_count=-1), E_INV), (dict(begin=TOP, sample_count=1), E_INV), (dict(first=TOP - n + 1), E_INV),
             (dict(num_rays=0x80000000), E_INV), (dict(first=0xffffffff), E_INV),
             (dict(num_triangles=-1), E_INV), (dict(num_materials=0), E_INV), (dict(nl=-1), E_INV), (dict(nl=1 << 24), E_INV),
             (dict(light_samples=0), E_INV), (dict(light_samples=257), E_INV), (dict(max_bounces=0), E_INV), (dict(max_bounces=65536), E_INV),
             (dict(reserved=0), E_INV), (dict(reserved=5), E_INV),
             (dict(num_triangles=raw.ntri + 1), E_RANGE), (dict(num_materials=raw.nmat + 1), E_RANGE), (dict(nl=len(raw.lights) + 1), E_RANGE),
             (dict(num_rays=NMAX + 1), E_RANGE)]
    for kw, code in cases:
        assert raw.call(raw.params(n, 2, **kw), **est) == code, kw
    p = raw.params(n, 2)
    assert raw.call(None) == E_INV
    assert raw.call(p, rr=None) == E_INV
    for rr in ((0, 0.9), (2, 0.0), (2, 1.5), (2, float("nan"))):
        assert raw.call(p, rr=rr) == E_INV, rr
    assert raw.call(p, mis=2) == E_INV
    for name in ("tb", "mb", "rb", "sb"):
        assert raw.call(p, **{name: None}, **est) == E_INV, name
    assert raw.call(p, lb=None) == E_INV                                    # num_lights > 0 needs the list,
    assert raw.call(p, mis=True, cb=None) == E_INV                          # MIS the counts,
    assert raw.call(p, power=True, cdf=None) == E_INV and raw.call(p, power=True, triq=None) == E_INV   # the table both halves
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    ob = adl.Buffer(other, 56 * n, np.uint8)
    big = adl.Buffer(device, 1 << 16, np.uint8)
    try:
        assert raw.call(p, rb=ob) == E_INV and raw.call(p, qb=ob) == E_INV and raw.call(p, sb=ob) == E_INV   # another device's buffers

        def wrap(off, nbytes):                                              # sub-ranges of one allocation
            w = adl.Buffer()
            w.setRawPtr(device, big.m_ptr + off, nbytes)
            return w
        wraps = dict(r_short=wrap(0, 32 * n - 1), q_short=wrap(0, 56 * n - 1), s_short=wrap(0, 12 * n - 1), s_one=wrap(0, 12 * n),
                     r8=wrap(8, 32 * n), q4=wrap(4, 56 * n), s2=wrap(2, 24 * n),
                     r0=wrap(0, 32 * n), s_on_r=wrap(32 * n - 16, 24 * n), q_on_r=wrap(32 * n - 8, 56 * n), q0=wrap(16384, 56 * n),
                     s_on_q=wrap(16384 + 56 * n - 4, 24 * n), s_far=wrap(32768, 24 * n))
        try:
            assert raw.call(p, rb=wraps["r_short"]) == E_RANGE
            assert raw.call(p, qb=wraps["q_short"]) == E_RANGE
            assert raw.call(p, sb=wraps["s_short"]) == E_RANGE              # less than one sample of every ray
            assert raw.call(p, sb=wraps["s_one"], qb=None) == E_RANGE       # one sample of two, and no moments to take it
            assert raw.call(p, rb=wraps["r8"]) == E_INV and raw.call(p, qb=wraps["q4"]) == E_INV and raw.call(p, sb=wraps["s2"]) == E_INV
            assert raw.call(p, rb=wraps["r0"], sb=wraps["s_on_r"]) == E_INV
            assert raw.call(p, rb=wraps["r0"], qb=wraps["q_on_r"], sb=wraps["s_far"]) == E_INV
            assert raw.call(p, qb=wraps["q0"], sb=wraps["s_on_q"]) == E_INV
            assert raw.call(p, rb=raw.lb) == E_RANGE                        # (the list is too small to be the rays)
            assert raw.call(raw.params(1, 1), rb=raw.cdf, power=True) == E_INV   # the rays on a light buffer
            assert raw.call(raw.params(1, 1), sb=raw.cb, mis=True) == E_INV      # the samples on one
        finally:
            for w in wraps.values():
                w.release()
    finally:
        big.release()
        ob.release()
        adl.DeviceUtils.deallocate(other)
    raw.assert_untouched("argument errors")


class _Probe:
    """a RadianceCaster in a renderer's shape: one sample of 1 031 rays through the soup"""

    def __init__(self, device):
        tris = scenes.soup(2000)
        mats = np.zeros(7, scene.MATERIAL_DTYPE)
        mats["albedo"][:, :3] = 0.5
        mats["emissive"][5, :3] = 2.0
        self.c = radiance.RadianceCaster(device, tris, mats, max_bounces=3, mis=True, light_choice="power", roulette=2)
        self.R, self.out = _soup_rays(tris, 1031, 4), None

    def render(self, frames, frame_begin=0):
        self.out = self.c.radiance(self.R, frames, sample_begin=frame_begin)

    def read(self):
        return self.out.mean

    def release(self):
        self.c.release()


def test_a_cut_short_search_is_reported(device):
    assert_cut_short_search_is_reported(device, lambda: _Probe(device))


def _resolved(mom):
    mean, v = moments_oracle.resolve(mom)
    with np.errstate(over="ignore"):
        return mean.astype(np.float32), v.astype(np.float32)


def test_caster_numpy_and_torch_agree_with_the_abi(device, cornell, raw_cornell):
    import torch

    tris, mats = cornell
    R, _ = _cornell_case(cornell, True, True)
    _, mom = raw_cornell.run(R, 5, mis=True, power=True, first=21, begin=2)
    mean, var = _resolved(mom)
    c = radiance.RadianceCaster(device, tris, mats, light_samples=K, max_bounces=B, mis=True, light_choice="power", roulette=Roulette(*RR),
                                workspace_bytes=12 * NMAX * 2)   # (chunks of 2, 2 and 1)
    try:
        got = c.radiance(R, 5, first_ray=21, sample_begin=2)
        for form, res in (("numpy", got), ("RAY_DTYPE", c.radiance(R.view(radiance.RAY_DTYPE).reshape(-1), 5, first_ray=21, sample_begin=2))):
            assert res.mean.dtype == np.float32 and res.n.dtype == np.uint32 and res.mean.shape == (NMAX, 3)
            assert_fb_equal(res.mean, mean, form + ": mean")
            assert_fb_equal(res.variance, var, form + ": variance")
            assert np.array_equal(res.n, mom["n"]) and np.array_equal(res.rejected, mom["rejected"]), form
        dev = "cuda:%d" % device.m_deviceIdx
        t = c.radiance(torch.from_numpy(R).to(dev), 5, first_ray=21, sample_begin=2)
        assert t.mean.is_cuda and t.mean.dtype == torch.float32 and tuple(t.mean.shape) == (NMAX, 3)
        assert_fb_equal(t.mean.cpu().numpy(), mean, "torch: mean")
        assert_fb_equal(t.variance.cpu().numpy(), var, "torch: variance")
        assert np.array_equal(t.n.cpu().numpy().view(np.uint32), mom["n"]) and np.array_equal(t.rejected.cpu().numpy().view(np.uint32), mom["rejected"])
        # accumulate: two calls equal one, in both forms
        c.radiance(R, 2, first_ray=21, sample_begin=2)
        two = c.radiance(R, 3, first_ray=21, sample_begin=4, accumulate=True)
        assert_fb_equal(two.mean, mean, "accumulate: mean")
        assert_fb_equal(two.variance, var, "accumulate: variance")
        assert np.array_equal(two.n, mom["n"])
        rt = torch.from_numpy(R).to(dev)
        c.radiance(rt, 2, first_ray=21, sample_begin=2)
        two = c.radiance(rt, 3, first_ray=21, sample_begin=4, accumulate=True)
        assert_fb_equal(two.mean.cpu().numpy(), mean, "torch, accumulate: mean")
        assert_fb_equal(two.variance.cpu().numpy(), var, "torch, accumulate: variance")
        with pytest.raises(ValueError):
            c.radiance(R, 1, accumulate=True)                      # the last call was a torch one
        with pytest.raises(ValueError):
            c.radiance(R, 1, sample_begin=TOP)
        with pytest.raises(TypeError):
            c.radiance(R[:, :7], 1)
        empty = c.radiance(R[:0], 3)
        assert empty.mean.shape == (0, 3) and empty.n.shape == (0,)
    finally:
        c.release()


def test_a_renderers_caster_shares_its_scene(device):
    tris, mats = scenes.soup(2000), np.zeros(7, scene.MATERIAL_DTYPE)
    mats["albedo"][:, :3] = 0.5
    mats["emissive"][5, :3] = 2.0
    R = _soup_rays(tris, 257, 6)
    lib = shim.load()
    with options(device, ACCEL=2):
        r = IndirectRenderer(device, tris, mats, 16, 16, max_bounces=3, mis=True, light_choice="power", roulette=2, light_samples=2)
        own = radiance.RadianceCaster(device, tris, mats, max_bounces=3, mis=True, light_choice="power", roulette=2, light_samples=2)
        c = r.radiance_caster()
        try:
            r.render(2)
            r.read()
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            got = c.radiance(R, 3)
            r.render(1)
            r.read()
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds, "a second LBVH was built"
            assert c.tbuf is r.tbuf and c.counts is r.counts and c.cdf is r.cdf and c.tri_q is r.tri_q and c.lbuf is r.lbuf
            want = own.radiance(R, 3)
            assert_fb_equal(got.mean, want.mean, "the renderer's caster against a caster of its own")
            assert_fb_equal(got.variance, want.variance, "variance")
        finally:
            c.release()
            own.release()
            r.release()
        assert r.tbuf is None
