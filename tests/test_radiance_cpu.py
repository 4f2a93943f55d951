"""The CPU restatement of pt_radiance_rays (tests/rays_oracle.py) pinned without a device, and the Python argument checks of
oclpathtracer_amd.radiance that need none:

  * with B = 1 and no lights a sample is the emitted light of the surface the ray's closest search finds -- 3 x emissive of the
    material that query_oracle's closest hit names, clamped at 0 as shading clamps it -- and (0.45, 0.45, 0.45) on a miss: the sample
    start is pinned against the query restatement, independently of the estimators;
  * the seed identity: ray r at first_ray = a is ray 0 of a call with first_ray = a + r, for every estimator;
  * check_range and panorama_rays.
"""
import numpy as np
import pytest

import gpu_support
import query_oracle
import rays_oracle
from conftest import assert_fb_equal
from oclpathtracer_amd import radiance, scene
from oclpathtracer_amd.query import RAY_DTYPE

ESTIMATORS = [(False, False), (True, False), (False, True), (True, True)]   # (mis, power)


def _emitted(tris, mats, R):
    """what a path of one vertex and no light sample gathers along each ray, from the query restatement's closest hit"""
    far = np.array(R, np.float32).reshape(-1, 8)
    far[:, 3] = np.float32(1e20)                                   # (a radiance ray is unbounded: the query must not stop short)
    hit = query_oracle.closest(tris, far)
    tri = hit[:, 1].view(np.int32)
    want = np.full((len(far), 3), np.float32(0.45), np.float32)
    on = tri >= 0
    emi = mats["emissive"][tris["id"][tri[on]], :3]
    want[on] = np.maximum(np.float32(0.0) + np.float32(1.0) * emi * np.float32(3.0), np.float32(0.0))
    return want, on


def test_one_vertex_without_lights_is_the_emission_at_the_closest_hit(cornell):
    tris, mats = cornell
    R = gpu_support.cornell_rays(np.random.default_rng(5), 600, tris)
    lamp = scene.emitters(tris, mats)                              # the first 40 rays start inside the box: aim them at the lamp
    centre = (tris["p1"][lamp[0], :3] + tris["p2"][lamp[0], :3] + tris["p3"][lamp[0], :3]) / np.float32(3.0)
    R[:40, 4:7] = centre - R[:40, :3]
    R[::7, 3] = np.float32(1e-3)                                   # tmax is not read ...
    R[1::7, 3] = np.float32(np.nan)
    R[2::7, 3] = np.float32(0.0)
    R[:, 7] = np.arange(len(R), dtype=np.int32).view(np.float32)   # ... nor is reserved
    want, on = _emitted(tris, mats, R)
    assert on.sum() > 200 and (~on).sum() > 50, (on.sum(), (~on).sum())
    assert (want[:40].max(axis=1) > 0.45).sum() >= 10, "hardly a ray sees the lamp"
    for first_ray, sample_begin in ((0, 0), (1000, 5)):
        ws = rays_oracle.workspace(tris, mats, R, 2, 1, 1, sample_begin=sample_begin, first_ray=first_ray, lights=[])
        assert ws.shape == (2, len(R), 3)
        for s in range(2):
            assert_fb_equal(ws[s], want, "sample %d from ray id %d" % (s, first_ray))


@pytest.mark.parametrize("mis,power", ESTIMATORS)
def test_a_ray_is_its_id_and_its_sample_number(cornell, mis, power):
    tris, mats = cornell
    R = gpu_support.cornell_rays(np.random.default_rng(6), 30, tris)
    a, kw = 77, dict(mis=mis, power=power, sample_begin=3)
    whole = rays_oracle.workspace(tris, mats, R, 3, 2, 4, (2, 0.9), first_ray=a, **kw)
    assert np.unique(whole.reshape(-1, 3), axis=0).shape[0] > 40, "the samples do not differ"
    for r in (0, 11, 29):
        one = rays_oracle.workspace(tris, mats, R[r:r + 1], 3, 2, 4, (2, 0.9), first_ray=a + r, **kw)
        assert_fb_equal(one[:, 0], whole[:, r], "ray %d" % r)
    # ... and the samples of a later range are the later samples
    later = rays_oracle.workspace(tris, mats, R, 1, 2, 4, (2, 0.9), first_ray=a, mis=mis, power=power, sample_begin=5)
    assert_fb_equal(later[0], whole[2], "sample 5")
    # another id is another stream
    other = rays_oracle.workspace(tris, mats, R, 3, 2, 4, (2, 0.9), first_ray=a + 1, **kw)
    assert not np.array_equal(other, whole)


def test_the_table_is_cleared_and_checked():
    L = rays_oracle.lib()
    assert L.orays_set(None, 1, 0) == -1 and L.orays_set(None, 0, 0x7fffffff) == 0 and L.orays_set(None, 0, 0x80000000) == -1
    with pytest.raises(ValueError):
        with rays_oracle.rays(np.zeros((2, 8), np.float32), 0x7fffffff - 1):
            pass


def test_check_range():
    radiance.check_range(10, 4)
    radiance.check_range(0, 0, 0x7fffffff, 0x7fffffff)
    radiance.check_range(1, 1, 0x7fffffff - 1, 0x7fffffff - 1)
    for bad in (dict(samples=-1), dict(sample_begin=-1), dict(first_ray=-1), dict(samples=1.5), dict(samples=True),
                dict(samples=2, sample_begin=0x7fffffff - 1), dict(num_rays=2, first_ray=0x7fffffff - 1)):
        kw = dict(num_rays=1, samples=1, sample_begin=0, first_ray=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            radiance.check_range(**kw)


def test_panorama_rays():
    W, H = 16, 8
    r = radiance.panorama_rays((1.0, 2.0, 3.0), W, H)
    assert r.dtype == RAY_DTYPE and r.shape == (W * H,)
    assert np.array_equal(r["origin"], np.broadcast_to(np.float32([1, 2, 3]), (W * H, 3))) and np.all(r["tmax"] == np.float32(1e20))
    d = r["dir"].astype(np.float64).reshape(H, W, 3)
    assert np.allclose(np.linalg.norm(d, axis=2), 1.0, atol=1e-6)
    assert np.all(np.diff(d[:, 0, 1]) < 0) and d[0, 0, 1] > 0.97 and d[-1, 0, 1] < -0.97     # rows: from up to down
    mid = d[H // 2]
    # the centre column looks along -z, the first along +z: half a pixel off in both angles, cos(pi / 16) cos(pi / 16) = 0.962
    assert mid[W // 2, 2] < -0.96 and abs(mid[W // 2, 0]) < 0.2 and mid[0, 2] > 0.96
    assert np.allclose(d.sum(axis=1)[:, [0, 2]], 0.0, atol=1e-5)                             # a full turn
    for bad in ((0, 4), (4, 0), (65536, 65536)):
        with pytest.raises(ValueError):
            radiance.panorama_rays((0, 0, 0), *bad)
    for eye in ((0, 0), (0, np.nan, 0)):
        with pytest.raises(ValueError):
            radiance.panorama_rays(eye, 4, 4)
