"""Batched ray queries on the MI355X (pt_intersect_rays, pt_camera_rays) against the CPU oracle, bit for bit.

"Bit-exact" is assert_fb_equal's: NaN masks equal, every other bit equal.  The oracle side is tests/query_oracle.c, which runs
the oracle's own getRay and triangle test in ascending order with hitDistance starting at min(tmax, 1e20)."""
import ctypes

import numpy as np
import pytest

import camera_oracle
import query_oracle as qo
from conftest import assert_fb_equal
from gpu_support import SEARCHES, assert_hits_equal, cornell_rays, options, refill_rays
from oclpathtracer_amd import shim
from scenes import horizon_tiles, soup_with_duplicates

pytestmark = pytest.mark.gpu


def _query_both(rc, rays, what):
    """closest and occluded of float32 [N, 8] rays through the numpy path; checks occluded == (tri >= 0)."""
    from oclpathtracer_amd import query

    hits = rc.closest(rays.view(query.RAY_DTYPE).reshape(-1))
    occ = rc.occluded(rays)
    assert occ.dtype == np.int32
    assert np.array_equal(occ, (hits["tri"] >= 0).astype(np.int32)), "%s: occluded != (closest.tri >= 0)" % what
    return hits


@pytest.mark.parametrize("quad,accel", SEARCHES)
def test_cornell_random_rays_bit_exact(device, cornell, quad, accel):
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(100 + quad + 10 * accel), 20480, tris)
    want = qo.closest(tris, rays)
    assert (want[:, 1].view(np.int32) >= 0).mean() > 0.3
    rc = RayCaster(device, tris)
    try:
        with options(device, QUAD_FILTER=quad, ACCEL=accel):
            got = _query_both(rc, rays, "cornell q%d a%d" % (quad, accel))
    finally:
        rc.release()
    assert_hits_equal(got, want, "cornell q%d a%d" % (quad, accel))
    hit = got["tri"] >= 0
    assert np.array_equal(got["material"][hit], tris["id"][got["tri"][hit]])
    assert np.all(got["t"][~hit] == np.inf) and np.all(got["material"][~hit] == -1)


def test_closest_agrees_with_intersect_world(device, cornell, oracle):
    """the oracle's own intersect_world (t, p, n, triangle) on a sample of rays"""
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(7), 600, tris)
    rc = RayCaster(device, tris)
    try:
        got = rc.closest(rays)
    finally:
        rc.release()
    for k in range(len(rays)):
        hit, t, p, n, tri = oracle.intersect_world(tris, rays[k, :3], rays[k, 4:7])
        assert got["tri"][k] == tri
        if hit:
            assert_fb_equal(np.concatenate([[got["t"][k]], got["p"][k], got["n"][k]]),
                            np.concatenate([[np.float32(t)], p, n]), "ray %d" % k)


@pytest.mark.parametrize("accel", [1, 2])
def test_soup_and_duplicates_bit_exact(device, accel):
    from oclpathtracer_amd.query import RayCaster

    tris = soup_with_duplicates(3000, 11)
    rng = np.random.default_rng(12)
    n = 8192
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-5, 5, (n, 3))
    r[:, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    # rays aimed at the duplicated triangles' centroids
    dup = rng.integers(10, 50, 512)
    cen = (tris["p1"][dup, :3] + tris["p2"][dup, :3] + tris["p3"][dup, :3]) / np.float32(3)
    r[:512, 4:7] = cen - r[:512, :3]
    want = qo.closest(tris, r)
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=accel):
            got = _query_both(rc, r, "soup a%d" % accel)
    finally:
        rc.release()
    assert_hits_equal(got, want, "soup a%d" % accel)
    assert not np.any((got["tri"] >= 1500) & (got["tri"] < 1540)), "a duplicate beat its lower-index original"


def test_edge_on_coplanar_tiles_through_the_lbvh(device):
    from oclpathtracer_amd.query import RayCaster

    tris, _ = horizon_tiles(0.003)
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=2):
            cam = rc.camera_rays(96, 64, 3)
            rays = cam.view(np.float32).reshape(-1, 8).copy()
            rng = np.random.default_rng(3)
            g = np.zeros((4096, 8), np.float32)                  # grazing rays just above the plane
            g[:, 0], g[:, 1], g[:, 2] = rng.uniform(-3, 3, 4096), 2.747 + rng.uniform(0, 1e-3, 4096), 4.0
            g[:, 3] = 1e20
            g[:, 4], g[:, 5], g[:, 6] = rng.uniform(-0.2, 0.2, 4096), -(10.0 ** rng.uniform(-5, -2, 4096)), -1.0
            rays = np.concatenate([rays, g])
            got = _query_both(rc, rays, "tiles")
    finally:
        rc.release()
    assert (got["tri"] >= 0).sum() > 2000
    assert_hits_equal(got, qo.closest(tris, rays), "edge-on tiles")


@pytest.mark.parametrize("accel", [1, 2])
def test_tmax_is_strict_and_clamped(device, cornell, accel):
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    base = cornell_rays(np.random.default_rng(21), 4096, tris)
    want = qo.closest(tris, base)
    hit = want[:, 1].view(np.int32) >= 0
    b = base[hit]
    t = want[hit, 0]
    at = b.copy()
    at[:, 3] = t                                                  # tmax == t_closest: that hit does not count
    above = b.copy()
    above[:, 3] = np.nextafter(t, np.float32(np.inf))             # the next float up: it does
    # tmax <= 0 or NaN; above 1e20; 1e20 itself; tiny positive ones (the LBVH's scaled-distance cap, a strict compare at a denormal)
    tiny = np.array([1e-30, 1e-40, 1.4e-45, 1e-3], np.float32)
    special = np.repeat(b[:64], 11, axis=0)
    special[:, 3] = np.tile(np.concatenate([np.array([0.0, -0.0, -1.0, np.nan, np.inf, 3e38, 1e20], np.float32), tiny]), 64)
    rays = np.concatenate([at, above, special])
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=accel):
            got = _query_both(rc, rays, "tmax a%d" % accel)
    finally:
        rc.release()
    assert_hits_equal(got, qo.closest(tris, rays), "tmax a%d" % accel)
    m = len(b)
    assert np.all(got["tri"][m: 2 * m] == want[hit, 1].view(np.int32))
    assert_fb_equal(got["t"][m: 2 * m], t, "nextafter")
    sp = got[2 * m:].reshape(64, 11)
    assert np.all(sp["tri"][:, :4] == -1) and np.all(sp["t"][:, :4] == np.inf)   # tmax <= 0 or NaN: a miss
    for k in (4, 5):                                                               # above 1e20: as 1e20
        assert np.array_equal(sp["tri"][:, k], sp["tri"][:, 6]) and np.array_equal(sp["t"][:, k], sp["t"][:, 6])


@pytest.mark.parametrize("accel", [1, 2])
def test_non_finite_and_degenerate_rays(device, cornell, accel):
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    inf, nan, den = np.float32(np.inf), np.float32(np.nan), np.float32(1e-40)
    vals = [0.0, -0.0, 1.0, -1.0, 0.3, 2.75, inf, -inf, nan, den, -den, 1e-30, 1e30, 3e38]
    rng = np.random.default_rng(4)
    n = 6000
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-3, 3, (n, 3))
    r[:, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    pick = rng.uniform(size=(n, 6)) < 0.3
    choice = np.array(vals, np.float32)[rng.integers(0, len(vals), (n, 6))]
    block = r[:, [0, 1, 2, 4, 5, 6]]
    block[pick] = choice[pick]
    r[:, [0, 1, 2, 4, 5, 6]] = block
    r[:100, 4:7] = 0.0                                                   # zero direction
    r[100:200, 4:7] = rng.normal(size=(100, 3)).astype(np.float32) * den  # denormal directions
    r[200:300, 4:7] = rng.normal(size=(100, 3)).astype(np.float32) * np.float32(1e25)   # |dir|^2 overflows
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=accel):
            got = _query_both(rc, r, "non-finite a%d" % accel)
    finally:
        rc.release()
    assert_hits_equal(got, qo.closest(tris, r), "non-finite a%d" % accel)


def test_empty_scene_and_zero_rays(device, cornell):
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.query import RayCaster

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(9), 512, tris)
    rc = RayCaster(device, np.zeros(0, scene.TRIANGLE_DTYPE))
    try:
        got = _query_both(rc, rays, "empty scene")
        assert np.all(got["tri"] == -1) and np.all(got["t"] == np.inf)
    finally:
        rc.release()
    rc = RayCaster(device, tris)
    try:
        assert len(rc.closest(np.zeros((0, 8), np.float32))) == 0
        assert len(rc.occluded(np.zeros((0, 8), np.float32))) == 0
    finally:
        rc.release()


def test_c_abi_argument_errors(device, cornell):
    from oclpathtracer_amd import adl, scene

    tris, _ = cornell
    lib = shim.load()
    tb = adl.Buffer(device, len(tris), scene.TRIANGLE_DTYPE)
    rb = adl.Buffer(device, 32 * 10, np.uint8)
    ob = adl.Buffer(device, 48 * 10, np.uint8)
    tb.write(tris, len(tris))
    rb.write(np.zeros(320, np.uint8), 320)
    try:
        call = lambda nt, n, mode, out=ob: lib.pt_intersect_rays(device._h, tb._h, nt, rb._h, out._h, n, mode, None)
        assert call(len(tris), 10, 0) == shim.PT_OK
        assert call(len(tris) + 1, 10, 0) == shim.PT_ERR_RANGE      # more triangles than the buffer holds
        assert call(len(tris), 11, 0) == shim.PT_ERR_RANGE          # more rays than the buffers hold
        assert call(len(tris), 10, 2) == shim.PT_ERR_INVALID        # no such mode
        assert call(-1, 10, 0) == shim.PT_ERR_INVALID
        assert call(len(tris), 10, 1) == shim.PT_OK                 # 40 bytes of results
        assert call(len(tris), 10, 0, rb) == shim.PT_ERR_RANGE      # 480 bytes do not fit the ray buffer
        assert lib.pt_intersect_rays(device._h, tb._h, len(tris), rb._h, rb._h, 10, 1, None) == shim.PT_ERR_INVALID  # overlap
        assert lib.pt_intersect_rays(device._h, None, len(tris), rb._h, ob._h, 10, 0, None) == shim.PT_ERR_INVALID
        bad = shim.Camera()
        lib.pt_camera_reference(ctypes.byref(bad))
        bad.center[:] = bad.eye[:]                                   # center == eye
        assert lib.pt_camera_rays(device._h, ctypes.byref(bad), 2, 5, 0, rb._h, None) == shim.PT_ERR_INVALID
        assert lib.pt_camera_rays(device._h, None, 2, 6, 0, rb._h, None) == shim.PT_ERR_RANGE
        assert lib.pt_camera_rays(device._h, None, 0, 6, 0, rb._h, None) == shim.PT_ERR_INVALID
        assert lib.pt_camera_rays(device._h, None, 2, 5, 0, rb._h, None) == shim.PT_OK
        device.waitForCompletion()
    finally:
        for b in (tb, rb, ob):
            b.release()


def _moved_cameras():
    from oclpathtracer_amd.camera import Camera

    return [Camera.reference(),
            Camera(eye=(1.0, 3.5, 6.0), center=(-0.5, 2.0, -1.0), up=(0.0, 1.0, 0.0), fov_y_deg=45.0),
            Camera(eye=(-2.0, 1.0, 3.0), center=(1.0, 3.0, -2.0), up=(0.1, 1.0, 0.0), fov_y_deg=75.0),
            Camera(eye=(0.3, 4.5, 2.0), center=(0.0, 0.5, -3.0), up=(0.0, 0.0, -1.0), fov_y_deg=30.0)]


def test_camera_rays_are_the_renderers_primary_rays(device, cornell, oracle):
    from oclpathtracer_amd.query import RayCaster

    tris, mats = cornell
    W, H = 64, 48
    rc = RayCaster(device, tris)
    try:
        for cam in _moved_cameras():
            got = rc.camera_rays(W, H, 5, cam)
            want = qo.camera_rays(W, H, 5, cam)
            assert_fb_equal(got.view(np.float32).reshape(-1, 8), want, "camera rays %s" % (cam,))
            assert np.all(got["origin"] == np.asarray(cam.eye, np.float32))
            assert np.all(got["tmax"] == np.float32(1e20))
        assert_fb_equal(rc.camera_rays(W, H, 5).view(np.float32).reshape(-1, 8), qo.camera_rays(W, H, 5), "camera=None")
        gids = np.arange(W * H, dtype=np.int32)
        for f in (0, 1, 7):
            rays = rc.camera_rays(W, H, f)
            # the reference's own generateRay for a few pixels: origin and getRay's direction
            for gid in (0, 1, W * H // 2 + 3, W * H - 1):
                o, d, _ = oracle.generate_ray(gid % W, gid // W, W, H, gid + oracle.hash_u32(f))
                assert_fb_equal(rays["origin"][gid], o, "origin")
                n = rc.closest(rays[gid: gid + 1])
                assert n["tri"][0] == oracle.intersect_world(tris, o, d)[4]
            first = rc.closest(rays)["tri"]
            _, hits = oracle.paths(tris, mats, gids, np.full(W * H, f, np.int32), W, H)
            assert np.array_equal(first, hits[:, 0]), "frame %d: %d first hits differ" % (f, int((first != hits[:, 0]).sum()))
    finally:
        rc.release()


def test_queries_interleaved_with_checkpointed_renders(device, cornell, oracle):
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.render import Renderer

    tris, mats = cornell
    W = H = 32
    lib = shim.load()
    rays = cornell_rays(np.random.default_rng(31), 4096, tris)
    want = qo.closest(tris, rays)
    with options(device, ACCEL=2, CHUNK_FRAMES=3):
        r = Renderer(device, tris, mats, W, H, want_stats=True)
        rc = r.ray_caster()
        try:
            r.render(4)
            assert_hits_equal(rc.closest(rays), want, "after render 1")
            builds = lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT)
            ws = device.getWorkspaceMemory()
            r.render(4)
            occ = rc.occluded(rays)
            r.render(3)
            assert_hits_equal(rc.closest(rays), want, "after render 3")
            assert np.array_equal(occ, (want[:, 1].view(np.int32) >= 0).astype(np.int32))
            assert int(r.read_stats_raw()[shim.PT_STAT_CARRIED]) > 0, "no launch was checkpointed"
            assert_fb_equal(r.read(), oracle.render(tris, mats, W, H, 11), "pixels after interleaved queries")
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds
            assert device.getWorkspaceMemory() == ws
            # a moved camera after queries: the render follows the camera oracle, and later queries stay exact
            cam = Camera(eye=(1.0, 3.5, 6.0), center=(-0.5, 2.0, -1.0), up=(0.0, 1.0, 0.0), fov_y_deg=45.0)
            r.set_camera(cam)
            r.render(3)
            assert_hits_equal(rc.closest(rays), want, "after the moved render")
            assert_fb_equal(r.read(), camera_oracle.render(tris, mats, W, H, 3, cam), "moved camera after a query")
            assert lib.pt_device_get_option(device._h, shim.PT_OPT_BVH_BUILD_COUNT) == builds
        finally:
            rc.release()
            r.release()


def test_cut_short_search_is_reported_and_recovers(device):
    from oclpathtracer_amd.query import RayCaster

    tris = soup_with_duplicates(3000, 41)
    rng = np.random.default_rng(42)
    n = 4096
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-5, 5, (n, 3))
    r[:, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=2):
            rc.closest(r[:64])                       # scene prepared, hierarchy built
            with options(device, BVH_STACK_LIMIT=1):
                with pytest.raises(shim.ShimError) as e:
                    rc.closest(r)
                assert e.value.code == shim.PT_ERR_TRAVERSAL
            device.waitForCompletion()               # the word was cleared by the report
            assert_hits_equal(rc.closest(r), qo.closest(tris, r), "stack limit back at 64")
    finally:
        rc.release()


def test_torch_tensors_in_and_out_without_host_sync(device, cornell):
    torch = pytest.importorskip("torch")
    from oclpathtracer_amd import query

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(51), 8192, tris)
    rc = query.RayCaster(device, tris)
    try:
        want = rc.closest(rays)
        want_occ = rc.occluded(rays)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            src = torch.from_numpy(rays).pin_memory().to("cuda", non_blocking=True)
            rt = src * 1.0                                     # produced on torch's stream, consumed by the query
            ht = rc.closest(rt)
            ot = rc.occluded(rt)
            rt.fill_(float("nan"))                             # after the query on torch's stream: must not reach it
            hc = ht.clone()                                    # consumed on torch's stream
            oc = ot.clone()
            cam = rc.camera_rays(64, 48, 2, as_tensor=True)
            camh = rc.closest(cam)
        s.synchronize()
        assert tuple(ht.shape) == (8192, 12) and ht.dtype == torch.float32 and ot.dtype == torch.int32
        assert_hits_equal(hc.cpu().numpy(), want, "torch path")
        assert np.array_equal(oc.cpu().numpy(), want_occ)
        assert_fb_equal(cam.cpu().numpy(), rc.camera_rays(64, 48, 2).view(np.float32).reshape(-1, 8), "camera rays tensor")
        assert_hits_equal(camh.cpu().numpy(), rc.closest(rc.camera_rays(64, 48, 2)), "camera rays through torch")
    finally:
        rc.release()


def test_configs4_soup_lbvh_matches_brute_force(device):
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.query import RayCaster

    tris, _ = scene.make_soup()
    rng = np.random.default_rng(61)
    n = 65536
    r = np.zeros((n, 8), np.float32)
    r[:, 0] = rng.uniform(-2.7, 2.7, n)
    r[:, 1] = rng.uniform(0.05, 5.4, n)
    r[:, 2] = rng.uniform(-5.5, 4.0, n)
    r[:, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=2):
            bvh = rc.closest(r)
            bvh_occ = rc.occluded(r)
        with options(device, ACCEL=1):
            brute = rc.closest(r)
    finally:
        rc.release()
    assert (bvh["tri"] >= 0).mean() > 0.5   # (the box is open towards the camera)
    assert_hits_equal(bvh, brute, "LBVH vs brute force, 10^6 triangles")
    assert np.array_equal(bvh_occ, (bvh["tri"] >= 0).astype(np.int32))
    assert_hits_equal(bvh[:256], qo.closest(tris, r[:256]), "LBVH vs oracle, 10^6 triangles")


def test_lbvh_refill_over_more_rays_than_the_grid(device):
    """The LBVH query kernel's waves serve several groups of rays each (2^20 rays > the persistent grid's lanes) and refill lanes
    from later groups: every ray's result is its own, dead rays miss, and the LBVH agrees with the brute force and the oracle."""
    from oclpathtracer_amd.query import RayCaster

    tris = soup_with_duplicates(3000, 71)
    n = 1 << 20
    grid_lanes = shim.load().pt_device_num_cus(device._h) * 5 * 256
    assert n > 2 * grid_lanes, "the test must give every wave of the grid more than one group"
    r = refill_rays(n, 72)
    dead = ~(r[:, 3] > 0)
    assert dead.mean() > 0.2
    rc = RayCaster(device, tris)
    try:
        with options(device, ACCEL=2):
            bvh = _query_both(rc, r, "refill a2")
        with options(device, ACCEL=1):
            brute = _query_both(rc, r, "refill a1")
    finally:
        rc.release()
    assert np.all(bvh["tri"][dead] == -1) and np.all(bvh["t"][dead] == np.inf) and np.all(bvh["material"][dead] == -1)
    assert (bvh["tri"][~dead] >= 0).mean() > 0.1
    assert_hits_equal(bvh, brute, "LBVH vs brute force, 2^20 rays")
    sample = np.concatenate([np.arange(0, n, 997), np.arange(n - 4096, n)])
    assert_hits_equal(bvh[sample], qo.closest(tris, r[sample]), "LBVH vs oracle, sampled")


class _Recorder:
    """Stands in for a device's ctypes library and records the names of the calls that go through it."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self.lib, name)

        def call(*a):
            self.calls.append(name)
            return f(*a)
        return call


def test_torch_calls_neither_free_nor_wait(device, cornell):
    """Many calls on device tensors, outputs kept or dropped: no buffer is freed (pt_buffer_free waits for the device), nothing
    waits on the host, the wraps are reused for recycled addresses, and the results are right."""
    torch = pytest.importorskip("torch")
    from oclpathtracer_amd import query

    tris, _ = cornell
    rays = cornell_rays(np.random.default_rng(81), 4096, tris)
    rc = query.RayCaster(device, tris)
    try:
        want = rc.closest(rays)
        rt = torch.from_numpy(rays).cuda()
        rec = _Recorder(device._lib)
        device._lib = rec
        try:
            kept = [rc.closest(rt) for _ in range(20)] + [rc.occluded(rt) for _ in range(20)]   # every output held
            kept_calls = list(rec.calls)
            rec.calls.clear()
            for _ in range(40):                                                                # outputs dropped
                h = rc.closest(rt)
            drop_calls = list(rec.calls)
        finally:
            device._lib = rec.lib
        waits = {"pt_buffer_free", "pt_sync", "pt_event_wait", "pt_event_elapsed_ns", "pt_buffer_map", "pt_buffer_read"}
        assert not waits & set(kept_calls + drop_calls), sorted(waits & set(kept_calls + drop_calls))
        assert drop_calls.count("pt_buffer_wrap") <= 4, "recycled addresses were wrapped again: %d" % drop_calls.count("pt_buffer_wrap")
        torch.cuda.synchronize()
        for h in kept[:20]:
            assert_hits_equal(h.cpu().numpy(), want, "kept output")
        for o in kept[20:]:
            assert np.array_equal(o.cpu().numpy(), (want["tri"] >= 0).astype(np.int32))
        assert_hits_equal(h.cpu().numpy(), want, "last dropped-loop output")
        # a tensor of another device is refused before anything is enqueued
        idx = device.m_deviceIdx
        device.m_deviceIdx = idx + 1
        try:
            with pytest.raises(ValueError):
                rc.closest(rt)
        finally:
            device.m_deviceIdx = idx
    finally:
        rc.release()
