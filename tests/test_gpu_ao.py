"""Ambient occlusion (pt_render_ao) and the early-exit occlusion search (pt_occluded_rays) on the MI355X, bit for bit.

The counts {open, hits} are compared with tests/ao_oracle.c, which composes the estimator from the CPU oracle's own camera ray,
triangle test (ascending loop) and hemisphere sampling; pt_occluded_rays is compared with pt_intersect_rays(PT_QUERY_OCCLUDED)."""
import ctypes

import numpy as np
import pytest

import ao_oracle as ao
from conftest import assert_fb_equal
from gpu_support import SEARCHES, cornell_rays, harness_ppm, options, refill_rays
from oclpathtracer_amd import shim
from scenes import edge_scene, soup_with_duplicates

pytestmark = pytest.mark.gpu


def _render(device, tris, W, H, frames, K, radius, frame_begin=0, **kw):
    from oclpathtracer_amd.ao import AORenderer

    r = AORenderer(device, tris, W, H, rays_per_sample=K, radius=radius, **kw)
    try:
        r.render(frames, frame_begin)
        return r.read_counts(), r.read_image()
    finally:
        r.release()


def _check_image(img, counts, K, miss=1.0, what=""):
    from oclpathtracer_amd.ao import resolve

    a = resolve(counts, K, miss).reshape(-1)
    want = np.stack([a, a, a, np.ones_like(a)], axis=1)
    assert_fb_equal(img, want, what + " image")


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_counts_bit_exact(device, cornell, quad, accel):
    tris, _ = cornell
    for W, H in ((64, 64), (40, 24)):
        for radius in (0.5, 1e20):
            want = ao.counts(tris, W, H, 0, 4, 8, radius)
            assert want[..., 1].sum() > 0 and (want[..., 0] < 8 * want[..., 1]).any()
            with options(device, QUAD_FILTER=quad, ACCEL=accel):
                got, img = _render(device, tris, W, H, 4, 8, radius, stripe_rows=1)
            what = "%dx%d r%g q%d a%d" % (W, H, radius, quad, accel)
            assert np.array_equal(got, want), what + ": counts differ at %d pixels" % int((got != want).any(-1).sum())
            _check_image(img, got, 8, 1.0, what)


@pytest.mark.parametrize("search,scene,accel", ao.SLAB_FORMS, ids=[f[0] for f in ao.SLAB_FORMS])
def test_unbounded_scene_that_shades(device, search, scene, accel):
    """pt_ao_kernel<false, ..> over the table in LDS and the tiled one, pt_ao_bvh_kernel<false, ..>: the boxes beside one triangle that
    lifts the scene over PT_DET_BOUND_MAX (scenes.slab), where samples hit, and rays are open and occluded (tests/test_ao_cpu.py)"""
    tris, _, _, cam = edge_scene(scene)[1]
    want = ao.slab_counts(scene)
    with options(device, QUAD_FILTER=0, ACCEL=accel):
        got, img = _render(device, tris, ao.SLAB_W, ao.SLAB_H, ao.SLAB_FRAMES, ao.SLAB_K, ao.SLAB_RADIUS, camera=cam, stripe_rows=1)
    assert np.array_equal(got, want), "%s: counts differ at %d pixels" % (scene, int((got != want).any(-1).sum()))
    _check_image(img, got, ao.SLAB_K, 1.0, scene)


def test_progressive_equals_one_call_and_frame_zero_overwrites(device, cornell):
    from oclpathtracer_amd.ao import AORenderer

    tris, _ = cornell
    W, H = 48, 40
    r = AORenderer(device, tris, W, H, rays_per_sample=4, radius=0.75, miss_value=-2.0, stripe_rows=1)
    try:
        garbage = np.full(2 * W * H, 0xDEADBEEF, np.uint32)
        r.counts.write(garbage, len(garbage))
        r.render(2)                       # frame 0: the garbage is overwritten
        r.render(3)                       # continues at frame 2
        assert r.frames_done == 5
        got = r.read_counts()
        img = r.read_image()
    finally:
        r.release()
    want = ao.counts(tris, W, H, 0, 5, 4, 0.75)
    assert np.array_equal(got, want)
    _check_image(img, got, 4, -2.0, "progressive")
    one, _ = _render(device, tris, W, H, 5, 4, 0.75, stripe_rows=1)
    assert np.array_equal(one, got)


def test_cameras_bit_exact_and_rejected_camera_enqueues_nothing(device, cornell):
    from oclpathtracer_amd import adl, scene
    from oclpathtracer_amd.camera import Camera

    tris, _ = cornell
    W, H = 48, 32
    cams = [Camera.fit(tris, view_dir=(0.3, -0.4, -1.0), aspect=W / H),
            Camera(eye=(-2.0, 1.0, 3.0), center=(1.0, 3.0, -2.0), up=(0.1, 1.0, 0.0), fov_y_deg=75.0)]
    for i, cam in enumerate(cams):
        want = ao.counts(tris, W, H, 0, 3, 6, 0.8, cam=cam)
        got, img = _render(device, tris, W, H, 3, 6, 0.8, camera=cam, stripe_rows=1)
        assert np.array_equal(got, want), "camera %d" % i
        _check_image(img, got, 6, 1.0, "camera %d" % i)
    lib = shim.load()
    tb = adl.Buffer(device, len(tris), scene.TRIANGLE_DTYPE)
    cb = adl.Buffer(device, 2 * W * H, np.uint32)
    tb.write(tris, len(tris))
    sentinel = np.full(2 * W * H, 0x5A5A5A5A, np.uint32)
    cb.write(sentinel, len(sentinel))
    try:
        bad = shim.Camera()
        lib.pt_camera_reference(ctypes.byref(bad))
        bad.center[:] = bad.eye[:]
        p = _params(W, H, len(tris))
        assert lib.pt_render_ao(device._h, tb._h, cb._h, None, ctypes.byref(p), ctypes.byref(bad), None) == shim.PT_ERR_INVALID
        back = np.zeros_like(sentinel)
        cb.read(back, len(back))
        device.waitForCompletion()
        assert np.array_equal(back, sentinel)
    finally:
        tb.release()
        cb.release()


def test_stripes_equal_the_single_rank_rows(device, cornell):
    from oclpathtracer_amd import adl
    from oclpathtracer_amd.ao import AORenderer

    tris, _ = cornell
    W, H, R, S = 40, 31, 3, 5
    full = AORenderer(device, tris, W, H, rays_per_sample=4, radius=0.6, stripe_rows=S)
    try:
        full.render(2)
        fc, fi = full.read_counts(), full.read_image()
    finally:
        full.release()
    lib = shim.load()
    slab = max(lib.pt_local_rows(H, S, R, k) for k in range(R))
    gathered = adl.Buffer(device, R * slab * W, adl.float4)
    image = adl.Buffer(device, W * H, adl.float4)
    try:
        for k in range(R):
            r = AORenderer(device, tris, W, H, rays_per_sample=4, radius=0.6, stripe_rows=S, n_ranks=R, rank=k)
            try:
                r.render(2)
                rows = (np.arange(H) // S) % R == k
                assert np.array_equal(r.read_counts(), fc[rows]), "rank %d" % k
                if r.local_pixels:
                    gathered.write(r.read_image(), r.local_pixels, k * slab * W)
            finally:
                r.release()
        shim.check(lib.pt_assemble_stripes(device._h, gathered._h, image._h, W, H, S, R, slab, None))
        out = np.zeros((W * H, 4), np.float32)
        image.read(out, W * H)
        device.waitForCompletion()
    finally:
        gathered.release()
        image.release()
    assert_fb_equal(out, fi, "assembled AO stripes")


def test_soup_lbvh_equals_brute_force(device):
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.camera import Camera

    tris, _ = scene.make_soup()
    cam = Camera.fit(tris)
    res = {}
    for accel in (2, 1):
        with options(device, ACCEL=accel):
            res[accel], _ = _render(device, tris, 64, 64, 1, 4, 1.0, camera=cam, stripe_rows=1)
    assert res[2][..., 1].sum() > 1000 and (res[2][..., 0] < 4 * res[2][..., 1]).any()
    assert np.array_equal(res[2], res[1])


# ---- pt_occluded_rays ---------------------------------------------------------------------------------------------------------
def _both(rc, rays):
    """PT_QUERY_OCCLUDED and the early-exit search of the same rays."""
    return rc.occluded(rays), rc.occluded(rays, early_exit=True)


def _tmax_rays(tris):
    """A hit exactly at tmax, tmax above 1e20, NaN, 0, -0, negative; non-finite and degenerate directions."""
    rng = np.random.default_rng(5)
    r = cornell_rays(rng, 2048, tris)
    r[0::7, 3] = np.float32(3e20)
    r[1::7, 3] = np.nan
    r[2::7, 3] = 0.0
    r[3::7, 3] = -0.0
    r[4::7, 3] = -1.0
    r[5::11, 4:7] = 0.0
    r[6::13, 4] = np.inf
    r[8::17, 5] = np.nan
    r[9::19, 4:7] = 1e-30
    return r


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_occluded_rays_equal_the_occluded_query(device, cornell, quad, accel):
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    rc = RayCaster(device, tris)
    try:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            rays = cornell_rays(np.random.default_rng(300 + quad + 10 * accel), 20480, tris)
            want, got = _both(rc, rays)
            assert want.mean() > 0.3 and np.array_equal(got, want)
            # hits exactly at tmax: the closest hit of each ray, then tmax = its t (strict: occluded must be 0)
            hits = rc.closest(rays)
            at = rays.copy()
            hit = hits["tri"] >= 0
            at[hit, 3] = hits["t"][hit]
            want, got = _both(rc, at)
            assert np.array_equal(got, want) and want[hit].sum() < hit.sum()
            want, got = _both(rc, _tmax_rays(tris))
            assert np.array_equal(got, want)
            assert len(rc.occluded(np.zeros((0, 8), np.float32), early_exit=True)) == 0
    finally:
        rc.release()


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_occluded_rays_hit_exactly_at_tmax_through_the_hierarchy(device, quad, accel):
    """A ray whose tmax is its own closest hit's t is not occluded (a hit counts at t < tmax); one whose tmax is the next float
    above is.  The 3 000-triangle soup's triangles are small against the scene, so they sit in the LBVH, not in its table of big
    triangles: with PT_OPT_ACCEL 2 the decision is pt_bvh_round's any-hit test, whose 64-bit key minimum would let a candidate AT
    tmax beat the incumbent."""
    from oclpathtracer_amd.query import RayCaster

    tris = soup_with_duplicates(3000, 81)
    rng = np.random.default_rng(82)
    n = 1 << 16
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-4, 4, (n, 3))
    r[:, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    rc = RayCaster(device, tris)
    try:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            hits = rc.closest(r)
            hit = hits["tri"] >= 0
            assert hit.sum() > 5000
            at = r.copy()
            at[hit, 3] = hits["t"][hit]
            want, got = _both(rc, at)
            assert want[hit].sum() < hit.sum()
            assert np.array_equal(got, want), "hit at tmax: %d rays differ" % int((got != want).sum())
            above = r.copy()
            above[hit, 3] = np.nextafter(hits["t"][hit], np.float32(np.inf))
            want, got = _both(rc, above)
            assert np.all(want[hit] == 1)
            assert np.array_equal(got, want), "hit just below tmax: %d rays differ" % int((got != want).sum())
    finally:
        rc.release()


def test_occluded_rays_empty_scene_and_edge_on_tiles(device, cornell):
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(8), 1024, tris)
    rc = RayCaster(device, np.zeros(0, scene.TRIANGLE_DTYPE))
    try:
        assert np.all(rc.occluded(rays, early_exit=True) == 0)
    finally:
        rc.release()
    # coplanar tiles met edge-on and at grazing angles through the LBVH
    n = 40
    g = np.zeros(2 * n * n, scene.TRIANGLE_DTYPE)
    k = 0
    for i in range(n):
        for j in range(n):
            a, b = np.array([i, 0, j], np.float32) * 0.1, np.array([i + 1, 0, j + 1], np.float32) * 0.1
            quad = [(a[0], 0, a[2]), (b[0], 0, a[2]), (b[0], 0, b[2]), (a[0], 0, b[2])]
            for tri in ((quad[0], quad[1], quad[2]), (quad[2], quad[3], quad[0])):
                for f, p in zip(("p1", "p2", "p3"), tri):
                    g[f][k, :3] = p
                k += 1
    rng = np.random.default_rng(77)
    m = 8192
    r = np.zeros((m, 8), np.float32)
    r[:, :3] = rng.uniform(-0.5, 4.5, (m, 3))
    r[: m // 2, 1] = 0.0                                                      # in the plane
    r[:, 3] = rng.choice(np.array([0.5, 2.0, 1e20], np.float32), m)
    r[:, 4:7] = rng.normal(size=(m, 3))
    r[: m // 4, 5] = 0.0                                                      # edge-on
    r[m // 2: 3 * m // 4, 5] = rng.choice(np.array([1e-6, -1e-6, -1.0], np.float32), m // 4)
    rc = RayCaster(device, g)
    try:
        for accel in (2, 1):
            with options(device, ACCEL=accel):
                want, got = _both(rc, r)
                assert np.array_equal(got, want), "tiles a%d" % accel
    finally:
        rc.release()


def test_occluded_rays_on_the_soup(device):
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.query import RayCaster

    tris, _ = scene.make_soup()
    rng = np.random.default_rng(2026)
    n = 1 << 22
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-1.2, 1.2, (n, 3))
    r[:, 4:7] = rng.normal(size=(n, 3))
    rc = RayCaster(device, tris)
    try:
        for tmax in (1.0, 1e20):
            r[:, 3] = tmax
            with options(device, ACCEL=2):
                want, got = _both(rc, r)
                assert np.array_equal(got, want), "soup LBVH tmax %g" % tmax
                assert 0.01 < want.mean() < 0.999
            small = r[: 1 << 14]
            for quad in (0, 1):
                with options(device, ACCEL=1, QUAD_FILTER=quad):
                    bw, bg = _both(rc, small)
                    assert np.array_equal(bg, bw) and np.array_equal(bg, want[: 1 << 14]), "soup brute q%d tmax %g" % (quad, tmax)
    finally:
        rc.release()


def test_occluded_rays_refill_over_more_rays_than_the_grid(device):
    from oclpathtracer_amd.query import RayCaster

    tris = soup_with_duplicates(3000, 71)
    r = refill_rays(1 << 20, 73)
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=2):
            want, got = _both(rc, r)
        assert np.array_equal(got, want) and np.all(got[~(r[:, 3] > 0)] == 0) and got.mean() > 0.05
    finally:
        rc.release()


def test_occluded_rays_through_torch_without_host_sync(device, cornell):
    torch = pytest.importorskip("torch")
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(61), 8192, tris)
    rc = RayCaster(device, tris)
    try:
        want = rc.occluded(rays)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            src = torch.from_numpy(rays).pin_memory().to("cuda", non_blocking=True)
            rt = src * 1.0
            ot = rc.occluded(rt, early_exit=True)
            rt.fill_(float("nan"))
            oc = ot.clone()
        s.synchronize()
        assert ot.dtype == torch.int32 and tuple(ot.shape) == (8192,)
        assert np.array_equal(oc.cpu().numpy(), want)
    finally:
        rc.release()


# ---- with renders, errors, the harness -----------------------------------------------------------------------------------------
def test_ao_interleaved_with_renders(device, cornell, oracle):
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    W = H = 32
    lib = shim.load()
    rays = cornell_rays(np.random.default_rng(33), 4096, tris)
    with options(device, ACCEL=2, CHUNK_FRAMES=3):
        r = Renderer(device, tris, mats, W, H, want_stats=True, stripe_rows=1)
        rc = r.ray_caster()
        a = r.ao_renderer(rays_per_sample=4, radius=0.9)
        try:
            r.render(7)                                          # checkpointed: 3 + 3 + 1 frames
            assert int(r.read_stats_raw()[shim.PT_STAT_CARRIED]) > 0
            assert_fb_equal(r.read(), oracle.render(tris, mats, W, H, 7), "render before AO")
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            a.render(2)
            ws = device.getWorkspaceMemory()
            want_occ = rc.occluded(rays)
            assert np.array_equal(rc.occluded(rays, early_exit=True), want_occ)
            a.render(2)
            r.render(4)
            assert_fb_equal(r.read(), oracle.render(tris, mats, W, H, 11), "render after AO and a query")
            assert np.array_equal(a.read_counts(), ao.counts(tris, W, H, 0, 4, 4, 0.9))
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds
            assert device.getWorkspaceMemory() == ws
        finally:
            a.release()
            rc.release()
            r.release()


def test_cut_short_search_is_reported_and_recovers(device):
    from oclpathtracer_amd.ao import AORenderer
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.query import RayCaster

    tris = soup_with_duplicates(3000, 41)
    rng = np.random.default_rng(43)
    n = 4096
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-5, 5, (n, 3))
    r[:, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    cam = Camera.fit(tris)
    with options(device, ACCEL=2):
        rc = RayCaster(device, tris)
        a = AORenderer(device, rc.tbuf, 48, 48, rays_per_sample=4, radius=2.0, camera=cam, num_triangles=len(tris), stripe_rows=1)
        try:
            want = rc.occluded(r)                          # scene prepared, hierarchy built
            a.render(1)
            want_ao = a.read_counts()
            for call in (lambda: rc.occluded(r, early_exit=True), lambda: (a.render(1, 0), a.read_counts())):
                with options(device, BVH_STACK_LIMIT=1):
                    with pytest.raises(shim.ShimError) as e:   # the search is cut short; the observing call reports it
                        call()
                    assert e.value.code == shim.PT_ERR_TRAVERSAL
                device.waitForCompletion()                     # the word was cleared by the report
            assert np.array_equal(rc.occluded(r, early_exit=True), want)
            a.render(1, 0)
            assert np.array_equal(a.read_counts(), want_ao)
        finally:
            a.release()
            rc.release()


def test_cpp_harness_ambient_occlusion(tmp_path, cornell):
    from oclpathtracer_amd import scene

    tris, _ = cornell
    _, name, pixels = harness_ppm(tmp_path, 64, 4, "AmbientOcclusion")
    assert name.startswith("ambientOcclusion_")
    from oclpathtracer_amd.ao import resolve
    a = resolve(ao.counts(tris, 64, 64, 0, 4, 16, 1.0), 16, 1.0).reshape(-1)
    assert np.array_equal(pixels, scene.f2c(np.stack([a, a, a], 1)))


def _params(W, H, ntri, **kw):
    p = shim.AoParams()
    p.width, p.height, p.frame_begin, p.frame_count = W, H, 0, 1
    p.num_triangles, p.rays_per_sample, p.radius, p.miss_value = ntri, 4, 1.0, 1.0
    p.stripe_rows, p.n_ranks, p.rank = 1, 1, 0
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    return p


def test_c_abi_argument_errors_leave_the_counts_untouched(device, cornell):
    from oclpathtracer_amd import adl, scene

    tris, _ = cornell
    lib = shim.load()
    W, H = 16, 8
    tb = adl.Buffer(device, len(tris), scene.TRIANGLE_DTYPE)
    cb = adl.Buffer(device, 2 * W * H + 16, np.uint32)
    ib = adl.Buffer(device, W * H + 4, adl.float4)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    ob = adl.Buffer(other, 2 * W * H, np.uint32)
    tb.write(tris, len(tris))
    sentinel = np.full(2 * W * H + 16, 0xA5A5A5A5, np.uint32)
    cb.write(sentinel, len(sentinel))
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    try:
        def call(p, counts=cb, image=ib, cam=None, tri=tb):
            return lib.pt_render_ao(device._h, tri._h if tri else None, counts._h if counts else None, image._h if image else None,
                                    ctypes.byref(p) if p is not None else None, cam, None)

        ntri = len(tris)
        cases = [(dict(width=0), E_INV), (dict(height=-1), E_INV), (dict(frame_begin=-1), E_INV), (dict(frame_count=-1), E_INV),
                 (dict(num_triangles=-1), E_INV), (dict(rays_per_sample=0), E_INV), (dict(rays_per_sample=257), E_INV),
                 (dict(radius=0.0), E_INV), (dict(radius=-1.0), E_INV), (dict(radius=float("inf")), E_INV), (dict(radius=float("nan")), E_INV),
                 (dict(miss_value=float("nan")), E_INV), (dict(miss_value=float("inf")), E_INV), (dict(stripe_rows=0), E_INV),
                 (dict(n_ranks=0), E_INV), (dict(rank=1), E_INV), (dict(rank=-1), E_INV), (dict(reserved=0), E_INV), (dict(reserved=4), E_INV),
                 (dict(frame_begin=0x7fffffff, frame_count=1), E_INV), (dict(width=65536, height=32768), E_INV),
                 (dict(num_triangles=ntri + 1), E_RANGE), (dict(width=W + 16), E_RANGE),
                 (dict(frame_begin=(1 << 24), frame_count=1, rays_per_sample=256), E_RANGE)]
        for kw, code in cases:
            p = _params(W, H, ntri, **kw)
            assert call(p) == code, kw
        p = _params(W, H, ntri)
        assert call(None) == E_INV
        assert call(p, tri=None) == E_INV and call(p, counts=None) == E_INV
        assert call(p, counts=ob) == E_INV                                   # a buffer of another device
        small_img = adl.Buffer(device, W * H - 1, adl.float4)
        try:
            assert call(p, image=small_img) == E_RANGE
        finally:
            small_img.release()
        bad = shim.Camera()
        lib.pt_camera_reference(ctypes.byref(bad))
        bad.fov_y_deg = 180.0
        assert call(p, cam=ctypes.byref(bad)) == E_INV
        # misaligned counts / image, counts and image overlapping: sub-ranges of one allocation
        big = adl.Buffer(device, 64 * W * H, np.uint8)
        try:
            base = big.m_ptr
            def wrap(off, nbytes):
                b = adl.Buffer()
                b.setRawPtr(device, base + off, nbytes)
                return b
            c4, i8, c0, i0 = wrap(4, 8 * W * H), wrap(8 * W * H + 8, 16 * W * H), wrap(0, 8 * W * H), wrap(8 * W * H - 16, 16 * W * H)
            try:
                assert call(p, counts=c4, image=None) == E_INV                # counts not 8-byte aligned
                assert call(p, counts=c0, image=i8) == E_INV                  # image not 16-byte aligned
                assert call(p, counts=c0, image=i0) == E_INV                  # overlap
            finally:
                for b in (c4, i8, c0, i0):
                    b.release()
        finally:
            big.release()
        back = np.zeros_like(sentinel)
        cb.read(back, len(back))
        device.waitForCompletion()
        assert np.array_equal(back, sentinel), "an argument error touched the counts"
        assert call(p) == shim.PT_OK
        device.waitForCompletion()
    finally:
        for b in (tb, cb, ib, ob):
            b.release()
        adl.DeviceUtils.deallocate(other)
