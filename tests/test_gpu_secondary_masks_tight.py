"""The refined builder of the secondary rays' masks (csrc/pt_secmask.h: adaptive boxes, the separating plane) on the device:
  (a) the device's table equals the host's at another stride than tests/test_gpu_secondary_masks.py takes, on scenes whose second mask
      word is in use: 64 triangles (the word full) and 34 (two bits of it).  The walk through the boxes diverges between the lanes of
      a wave and ends on a budget: equality of every compared entry is what says that the device walks as the host does.
      A scene of 33 triangles cannot stand on the device -- a table needs the quad pairing (pt_shim.hip: refresh_smask wants quad mode
      3), so an odd count declines it -- which is asserted; the host side of 33 triangles is tests/test_secondary_masks_tight_cpu.py;
  (b) renders at 96 x 64, 4 frames, depth 16 with the option 1 and 0 are bit-identical to each other and to the CPU oracle;
  (c) a 70 x 3 render: a partial last wave."""
import os
import subprocess

import numpy as np
import pytest

import scenes
from conftest import assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import scene as _scene, shim
from oclpathtracer_amd.camera import Camera
from oclpathtracer_amd.render import Renderer
from scenes import box_prefix, joined
from test_gpu_secondary_masks import no_table, oracle_rows, snapshot
from test_secondary_masks_cpu import records

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STRIDE = 1009   # (a prime, and not the 211 of tests/test_gpu_secondary_masks.py)


def far_cornell():
    """the box x 37.5, moved 80 away from the origin of coordinates (tests/test_secondary_masks_cpu.py), and the reference's view of it"""
    tris, mats = _scene.load_model()
    t = tris.copy()
    s, shift = np.float32(37.5), np.array([3.0, -80.0, 11.0], np.float32)
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = t[f][:, :3] * s + shift
    eye, to = np.array([0.0, 2.75, 4.0]) * 37.5 + shift, np.array([0.0, 2.75, 3.0]) * 37.5 + shift
    return t, mats, Camera(tuple(eye), tuple(to))


TABLES = {
    "sixty_four": lambda: joined(_scene.load_model(), scenes.random_quads(105), scenes.random_quads(1007)),
    "thirty_four": lambda: box_prefix(34),
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("secmask_tight_gpu")
    exe = str(d / "secondary_masks_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe,
                           os.path.join(HERE, "secondary_masks_check.cpp")])

    def table(tris):
        rec, out = str(d / "records.f32"), str(d / "table.u32")
        records(tris).tofile(rec)
        subprocess.check_call([exe, "table", rec, str(len(tris)), out, str(STRIDE)], stdout=subprocess.DEVNULL)
        return np.fromfile(out, np.uint32).reshape(-1, 2)

    def stands(tris):
        rec = str(d / "records.f32")
        records(tris).tofile(rec)
        return len(tris) <= 64 and subprocess.check_output([exe, "valid", rec, str(len(tris))]).decode().startswith("invalid 0 ")
    table.stands = stands
    return table


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_device_table_is_the_host_table_at_another_stride(device, host, name):
    tris, mats = TABLES[name]()
    assert len(tris) == {"sixty_four": 64, "thirty_four": 34}[name]
    render(device, tris, mats, 16, 16, 1, depth=2)
    assert not no_table(device), name + ": no table stands"
    got, info = snapshot(device)
    want = host(tris)
    assert info[1] == len(tris) and len(got) == len(tris) * info[2] ** 2 * 6 * info[3] ** 2
    some = got[::STRIDE]
    assert len(some) == len(want)
    diff = np.flatnonzero((some != want).any(axis=1))
    assert len(diff) == 0, "%d of %d entries differ (first: %d, device %s, host %s)" % (len(diff), len(want), diff[0] * STRIDE, some[diff[0]], want[diff[0]])
    assert got[:, 1].any(), "no entry uses the second mask word"
    if len(tris) < 64:
        assert (got[:, 1] >> (len(tris) - 32)).max() == 0, "bits above the scene's triangles"
    bits = np.unpackbits(got.view(np.uint8)).sum()
    print("%s: %d entries, %.2f candidates per entry of %d" % (name, len(got), bits / len(got), len(tris)))
    assert bits < len(got) * len(tris)


def test_thirty_three_triangles_decline_the_table(device):
    tris, mats = box_prefix(33)
    render(device, tris, mats, 16, 16, 1, depth=2)
    assert no_table(device), "an odd triangle count has no quad pairing, and the secondary masks need it"


# name: (scene -> (tris, mats[, camera]), W, H)
RENDERS = {
    "cornell": (_scene.load_model, 96, 64),
    "far_cornell": (far_cornell, 96, 64),
    "quads_105": (lambda: scenes.random_quads(105), 96, 64),
    "cornell_70x3": (_scene.load_model, 70, 3),
}


@pytest.mark.parametrize("name", list(RENDERS))
def test_option_on_and_off_and_the_oracle(device, oracle, host, name):
    make, W, H = RENDERS[name]
    frames, depth = 4, 16
    tris, mats, *rest = make()
    camera = rest[0] if rest else None
    stands = host.stands(tris)
    if name != "far_cornell":
        assert stands, name + ": the case is meant to render through the table"
    got = {}
    for on in (1, 0):
        with options(device, SECONDARY_MASKS=on):
            r = Renderer(device, tris, mats, W, H, camera=camera, want_stats=True)
            try:
                r.render(frames, max_bounces=depth)
                st = r.read_stats_raw()
                got[on] = (r.read(), int(st[shim.PT_STAT_RAYS]), int(st[shim.PT_STAT_SAMPLES]))
                rows, npix = r.global_rows(), r.local_pixels
                if on and name != "far_cornell":
                    assert not no_table(device), name + ": no table stands"
                if on:
                    print(name, "table stands:", not no_table(device))
            finally:
                r.release()
    want, rays = oracle_rows(oracle, tris, mats, W, H, frames, depth, camera, rows)
    for on in (1, 0):
        assert_fb_equal(got[on][0], want, "%s, secondary masks %d" % (name, on))
        assert got[on][1] == rays, "%s, secondary masks %d: %d rays, the oracle traced %d" % (name, on, got[on][1], rays)
        assert got[on][2] == npix * frames
    assert_fb_equal(got[1][0], got[0][0], name + ": on against off")
