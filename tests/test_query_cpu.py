"""Batched ray queries, host side (no GPU): record layouts, the Python argument checks, the torch layout of RAY_DTYPE."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_query_records_match_the_header():
    from oclpathtracer_amd import query, shim

    assert ctypes.sizeof(shim.Ray) == 32 and ctypes.sizeof(shim.Hit) == 48
    assert [(f, getattr(shim.Ray, f).offset) for f, _ in shim.Ray._fields_] == [("origin", 0), ("tmax", 12), ("dir", 16), ("reserved", 28)]
    assert [(f, getattr(shim.Hit, f).offset) for f, _ in shim.Hit._fields_] == [
        ("t", 0), ("tri", 4), ("u", 8), ("v", 12), ("p", 16), ("material", 28), ("n", 32), ("reserved", 44)]
    assert query.RAY_DTYPE.itemsize == 32 and query.HIT_DTYPE.itemsize == 48
    assert {k: v[1] for k, v in query.RAY_DTYPE.fields.items()} == {"origin": 0, "tmax": 12, "dir": 16, "reserved": 28}
    assert {k: v[1] for k, v in query.HIT_DTYPE.fields.items()} == {
        "t": 0, "tri": 4, "u": 8, "v": 12, "p": 16, "material": 28, "n": 32, "reserved": 44}
    assert shim.PT_QUERY_CLOSEST == 0 and shim.PT_QUERY_OCCLUDED == 1
    hdr = open(os.path.join(ROOT, "include", "pt_shim.h")).read()
    assert re.search(r"PT_QUERY_CLOSEST\s*=\s*0", hdr) and re.search(r"PT_QUERY_OCCLUDED\s*=\s*1", hdr)


def test_make_rays():
    from oclpathtracer_amd import query

    r = query.make_rays([[0, 1, 2], [3, 4, 5]], [[0, 0, -1], [1, 0, 0]], tmax=[5.0, 7.0])
    assert r.dtype == query.RAY_DTYPE and len(r) == 2
    words = r.view(np.float32).reshape(-1, 8)
    assert np.array_equal(words[:, :3], [[0, 1, 2], [3, 4, 5]]) and np.array_equal(words[:, 3], [5, 7])
    assert np.array_equal(words[:, 4:7], [[0, 0, -1], [1, 0, 0]]) and not words[:, 7].view(np.int32).any()
    assert np.all(query.make_rays(np.zeros((3, 3)), np.ones((3, 3)))["tmax"] == np.float32(1e20))
    with pytest.raises(ValueError):
        query.make_rays(np.zeros((3, 3)), np.ones((2, 3)))


def test_ray_dtype_round_trips_through_torch():
    torch = pytest.importorskip("torch")
    from oclpathtracer_amd import query

    rng = np.random.default_rng(5)
    r = query.make_rays(rng.normal(size=(17, 3)), rng.normal(size=(17, 3)), tmax=rng.uniform(0, 9, 17))
    r["reserved"] = np.arange(17)
    t = torch.from_numpy(r.view(np.float32).reshape(-1, query.RAY_WORDS))
    assert tuple(t.shape) == (17, 8) and t.dtype == torch.float32
    back = t.numpy().copy().view(query.RAY_DTYPE).reshape(-1)
    assert back.tobytes() == r.tobytes()
    assert np.array_equal(t[:, 7].view(torch.int32).numpy(), np.arange(17))


class _FakeDevice:
    """Stands in for an adl.Device: any call that would reach the library fails the test."""

    _h = None

    def __getattr__(self, name):
        raise AssertionError("argument checks must fail before %s is called" % name)


def _caster():
    from oclpathtracer_amd import adl, query

    rc = query.RayCaster.__new__(query.RayCaster)
    rc.dev = _FakeDevice()
    rc._lib = None          # nothing may be enqueued: a library call would raise AttributeError on None
    rc.tbuf = adl.Buffer()
    rc.num_triangles = 0
    rc._host, rc._wrapped, rc._sync, rc._own_tbuf = {}, {}, None, False
    return rc


@pytest.mark.parametrize("bad", [
    np.zeros((4, 7), np.float32),            # not 8 words
    np.zeros((4, 8), np.float64),            # not float32
    np.zeros(32, np.float32),                # flat
    np.zeros(4, [("a", "<f4")]),             # another record type
])
def test_python_checks_reject_bad_rays_before_anything_is_enqueued(bad):
    rc = _caster()
    with pytest.raises(TypeError):
        rc.closest(bad)
    with pytest.raises(TypeError):
        rc.occluded(bad)


def test_python_checks_reject_bad_tensors_before_anything_is_enqueued():
    torch = pytest.importorskip("torch")
    rc = _caster()
    with pytest.raises(TypeError):
        rc.closest(torch.zeros((4, 8), dtype=torch.float64))
    with pytest.raises(TypeError):
        rc.closest(torch.zeros((4, 6), dtype=torch.float32))
    with pytest.raises(ValueError):
        rc.closest(torch.zeros((4, 8), dtype=torch.float32))   # a host tensor


def test_python_checks_reject_bad_camera_ray_requests():
    rc = _caster()
    for w, h, f in ((0, 4, 0), (4, 0, 0), (4, 4, -1)):
        with pytest.raises(ValueError):
            rc.camera_rays(w, h, f)
    with pytest.raises(TypeError):
        rc.camera_rays(4, 4, 0, camera=(0, 0, 0))


def test_ray_caster_needs_a_triangle_count_with_a_buffer():
    from oclpathtracer_amd import adl, query

    with pytest.raises(ValueError):
        query.RayCaster(_FakeDevice(), adl.Buffer())
    with pytest.raises(TypeError):
        query.RayCaster(_FakeDevice(), np.zeros((3, 16), np.float32))
