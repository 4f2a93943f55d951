"""The secondary rays' candidate masks on the device (PT_OPT_SECONDARY_MASKS, csrc/pt_secmask.h), through the C ABI:
  (a) the table the trace kernel reads (pt_secondary_mask_snapshot) equals the one the host build of the same per-entry function
      makes (tests/secondary_masks_check.cpp): the builder works in binary64 without contraction on both sides, so equality is what
      is required of every entry compared: six WHOLE tiles (every direction cell of each: the first and last tile of the first and last
      triangle, two in the middle) and every STRIDE-th entry of the table.  A whole host table is minutes of one thread's time; for
      the entries not compared what is proved is containment: the device's whole table passes the CPU test's rays;
  (b) renders with the option 1 and 0 are bit-identical to each other and to the CPU oracle, ray and sample counts included;
  (c) a second scene replaces the table, a camera change leaves it alone, a scene that does not qualify declines it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import camera_oracle
import scenes
from conftest import assert_fb_equal
from gpu_support import options, render
from oclpathtracer_amd import scene as _scene, shim
from oclpathtracer_amd.camera import Camera
from oclpathtracer_amd.render import Renderer
from test_secondary_masks_cpu import records

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STRIDE = 211   # (a prime: the sample walks through every tile and direction cell)


def snapshot(device):
    lib = shim.load()
    info = (ctypes.c_uint32 * 4)()
    shim.check(lib.pt_secondary_mask_snapshot(device._h, info, None, 0))
    out = np.zeros((info[0], 2), np.uint32)
    shim.check(lib.pt_secondary_mask_snapshot(device._h, info, out.ctypes.data_as(ctypes.c_void_p), len(out)))
    return out, tuple(info)


def no_table(device):
    info = (ctypes.c_uint32 * 4)()
    return shim.load().pt_secondary_mask_snapshot(device._h, info, None, 0) == shim.PT_ERR_INVALID


@pytest.fixture(scope="module")
def host_table(tmp_path_factory):
    d = tmp_path_factory.mktemp("secmask_gpu")
    exe = str(d / "secondary_masks_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe,
                           os.path.join(HERE, "secondary_masks_check.cpp")])

    def make(tris):
        rec, out = str(d / "records.f32"), str(d / "table.u32")
        records(tris).tofile(rec)
        subprocess.check_call([exe, "table", rec, str(len(tris)), out, str(STRIDE)], stdout=subprocess.DEVNULL)
        return np.fromfile(out, np.uint32).reshape(-1, 2)

    def tile(tris, first, count):
        """entries first .. first + count - 1, one by one"""
        rec, out = str(d / "records.f32"), str(d / "tile.u32")
        records(tris).tofile(rec)
        subprocess.check_call([exe, "table", rec, str(len(tris)), out, "1", str(first), str(count)], stdout=subprocess.DEVNULL)
        return np.fromfile(out, np.uint32).reshape(-1, 2)
    make.tile = tile

    def rays(tris, table):
        """the CPU test's rays (its seed, 500 cells) against a whole table: the counters"""
        rec, tab = str(d / "records.f32"), str(d / "device.u32")
        records(tris).tofile(rec)
        np.ascontiguousarray(table, np.uint32).tofile(tab)
        r = subprocess.run([exe, "rays", rec, str(len(tris)), "20261020", "500", tab], capture_output=True, text=True, timeout=120)
        w = r.stdout.split()
        return r, dict(zip(w[0::2], (int(x) for x in w[1::2])))
    make.rays = rays

    def stands(tris):
        """whether the device keeps a table for the scene: at most 64 triangles, each with a table of its own (pt_sm_geom)"""
        if len(tris) > 64:
            return False
        rec = str(d / "records.f32")
        records(tris).tofile(rec)
        return subprocess.check_output([exe, "valid", rec, str(len(tris))]).decode().startswith("invalid 0 ")
    make.stands = stands
    return make


@pytest.mark.parametrize("name", ["cornell", "quads"])
def test_the_device_table_is_the_host_table(device, cornell, host_table, name):
    tris, mats = cornell if name == "cornell" else scenes.random_quads(126)   # (24 triangles, each with a table)
    assert len(tris) <= 64
    render(device, tris, mats, 16, 16, 1, depth=2)
    got, info = snapshot(device)
    want = host_table(tris)
    assert info[1] == len(tris) and info[0] == len(got) == len(tris) * info[2] ** 2 * 6 * info[3] ** 2
    some = got[::STRIDE]
    assert len(some) == len(want)
    diff = np.flatnonzero((some != want).any(axis=1))
    assert len(diff) == 0, "%d of %d entries differ (first: %d, device %s, host %s)" % (len(diff), len(want), diff[0] * STRIDE, some[diff[0]], want[diff[0]])
    dirs, tiles = 6 * info[3] ** 2, len(tris) * info[2] ** 2
    for t in (0, info[2] ** 2 - 1, tiles // 2, tiles // 2 + info[2] + 1, tiles - info[2] ** 2, tiles - 1):
        host = host_table.tile(tris, t * dirs, dirs)
        assert np.array_equal(got[t * dirs:(t + 1) * dirs], host), "tile %d of %d: %d of its %d entries differ" % (
            t, tiles, int((got[t * dirs:(t + 1) * dirs] != host).any(axis=1).sum()), dirs)
    r, c = host_table.rays(tris, got)
    assert r.returncode == 0 and c["missing"] == 0 and c["accepted"] > 0, r.stdout + r.stderr
    bits = np.unpackbits(got.view(np.uint8)).sum()
    print("%s: %d entries, %.2f candidates per entry of %d" % (name, len(got), bits / len(got), len(tris)))
    assert bits < len(got) * len(tris), "every entry keeps every triangle: the table says nothing"


def oracle_rows(oracle, tris, mats, W, H, frames, depth, camera, rows):
    """the oracle's image over the global rows ``rows`` and its ray count over them"""
    fb = np.zeros((H * W, 4), np.float32)
    rays = 0
    for run in np.split(rows, np.flatnonzero(np.diff(rows) != 1) + 1):
        kw = dict(fb=fb, gid_begin=int(run[0]) * W, gid_count=len(run) * W, max_bounces=depth, want_stats=True)
        _, st = oracle.render(tris, mats, W, H, frames, **kw) if camera is None else camera_oracle.render(tris, mats, W, H, frames, camera, **kw)
        rays += st["rays"]
    gids = (rows[:, None] * W + np.arange(W)[None, :]).reshape(-1)
    return fb[gids], rays


def scaled_cornell(s):
    tris, mats = _scene.load_model()
    t = tris.copy()
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = (tris[f][:, :3].astype(np.float64) * s).astype(np.float32)
    return t, mats, Camera((0.0, 2.75 * s, 4.0 * s), (0.0, 2.75 * s, 3.0 * s))


def sixty_six():
    """66 triangles of quads: the box and 15 quads of a shrunk copy inside it -- above the table's 64"""
    tris, mats = _scene.load_model()
    inner = tris[:30].copy()
    for f in ("p1", "p2", "p3"):
        inner[f][:, :3] = inner[f][:, :3] * np.float32(0.4) + np.array([0.3, 1.2, -1.9], np.float32)
    return np.concatenate([inner, tris]), mats


# name: (scene -> (tris, mats[, camera]), W, H, frames, depth, Renderer keywords, device options).  Whether a table stands is asked of the
# host build (host_table.stands): random quad scenes 105, 654 and 1240 keep one, 4 and 17 hold triangles without a table and decline it, as do
# the box x 1e-3 (every triangle smaller than the rays' offset) and the 66 triangles
CASES = {
    "cornell_d16": (_scene.load_model, 64, 64, 8, 16, {}, {}),
    "cornell_d2": (_scene.load_model, 64, 64, 8, 2, {}, {}),
    "cornell_33x97": (_scene.load_model, 33, 97, 3, 16, {}, {}),
    "cornell_rank1_of_3": (_scene.load_model, 64, 64, 4, 16, dict(n_ranks=3, rank=1, stripe_rows=4), {}),
    "cornell_chunks_of_2": (_scene.load_model, 64, 64, 8, 16, {}, dict(CHUNK_FRAMES=2)),
    "quads_105": (lambda: scenes.random_quads(105), 64, 64, 4, 16, {}, {}),
    "quads_654": (lambda: scenes.random_quads(654), 64, 64, 4, 16, {}, {}),
    "quads_1240": (lambda: scenes.random_quads(1240), 64, 64, 4, 16, {}, {}),
    "quads_4": (lambda: scenes.random_quads(4), 64, 64, 4, 16, {}, {}),
    "quads_17": (lambda: scenes.random_quads(17), 64, 64, 4, 16, {}, {}),
    "quads_25": (lambda: scenes.random_quads(25), 64, 64, 4, 16, {}, {}),
    "glossy_room": (scenes.glossy_room, 64, 48, 8, 16, {}, {}),
    "cornell_x1e3": (lambda: scaled_cornell(1e3), 64, 64, 4, 16, {}, {}),
    "cornell_x1e-3": (lambda: scaled_cornell(1e-3), 64, 64, 4, 16, {}, {}),
    "inside_up": (lambda: _scene.load_model() + (Camera((0.3, 1.5, -2.5), (0.0, 5.4, -2.8), up=(0.0, 0.0, -1.0)),), 64, 64, 4, 16, {}, {}),
    "sixty_six": (sixty_six, 48, 48, 3, 16, {}, {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_option_on_and_off_and_the_oracle(device, oracle, host_table, name):
    make, W, H, frames, depth, kw, opts = CASES[name]
    tris, mats, *rest = make()
    stands = host_table.stands(tris)
    if name.startswith("cornell_d") or name in ("quads_105", "quads_654", "quads_1240", "glossy_room", "inside_up"):
        assert stands, name + ": the case is meant to render through the table"
    camera = rest[0] if rest else None
    got = {}
    for on in (1, 0):
        with options(device, SECONDARY_MASKS=on, **opts):
            r = Renderer(device, tris, mats, W, H, camera=camera, want_stats=True, **kw)
            try:
                r.render(frames, max_bounces=depth)
                st = r.read_stats_raw()
                got[on] = (r.read(), int(st[shim.PT_STAT_RAYS]), int(st[shim.PT_STAT_SAMPLES]))
                rows, npix = r.global_rows(), r.local_pixels
                if on:
                    assert no_table(device) != stands, "%s: %s" % (name, "no table stands" if stands else "a table stands for a scene that declines it")
            finally:
                r.release()
    want, rays = oracle_rows(oracle, tris, mats, W, H, frames, depth, camera, rows)
    for on in (1, 0):
        assert_fb_equal(got[on][0], want, "%s, secondary masks %d" % (name, on))
        assert got[on][1] == rays, "%s, secondary masks %d: %d rays, the oracle traced %d" % (name, on, got[on][1], rays)
        assert got[on][2] == npix * frames
    assert_fb_equal(got[1][0], got[0][0], name + ": on against off")


def test_a_second_scene_replaces_the_table_and_a_camera_change_does_not(device, cornell):
    tris, mats = cornell
    lib = shim.load()
    quads, qmats = scenes.random_quads(126)
    render(device, quads, qmats, 16, 16, 1, depth=2)
    first, info1 = snapshot(device)
    r = Renderer(device, tris, mats, 32, 32)
    try:
        r.render(1)
        second, info2 = snapshot(device)
        assert info1[1] == len(quads) and info2[1] == len(tris)
        assert len(first) != len(second) or not np.array_equal(first, second), "the table did not follow the scene"
        ws = lib.pt_device_workspace_memory(device._h)
        r.set_camera(Camera((0.0, 2.75, 4.0), (-0.5, 2.75, 4.0 - 0.8660254)))
        r.render(1)
        third, _ = snapshot(device)
        assert np.array_equal(second, third), "a camera change altered the table"
        assert lib.pt_device_workspace_memory(device._h) == ws, "a camera change moved the workspace"
    finally:
        r.release()
    assert lib.pt_device_get_option(device._h, shim.PT_OPT_SECONDARY_MASKS) == 1
