"""The secondary rays' candidate masks (csrc/pt_secmask.h) against the reference's own test, on the host: the per-entry function the
device kernel runs is compiled by g++ into a stand-alone program (tests/secondary_masks_check.cpp, -ffp-contract=off as the library)
which samples cells, draws rays inside them -- tile corners and edges, the plane distance +-H, direction ratios on the cell's
boundary and one ulp to either side, directions grazing the origin triangle -- classifies each with the device's own classification
and requires that NO pair the reference accepts (oracle arithmetic, binary32) is missing from the mask of the ray's cell.  Rays the
classification does not cover are counted; that the trace kernel searches them with every triangle is what the GPU parity cases
(tests/test_gpu_secondary_masks.py) exercise.  At most 5 % of the sampled cells may go without a ray of their own."""
import os
import subprocess

import numpy as np
import pytest

import scenes
from oclpathtracer_amd import scene as _scene

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261020
CELLS = 2000


def records(tris):
    """the prepared records {p1, e1, e2} as the prep kernel stores them: binary32 differences"""
    n = len(tris)
    r = np.zeros((n, 16), np.float32)
    p1, p2, p3 = (tris[f][:, :3].astype(np.float32) for f in ("p1", "p2", "p3"))
    r[:, 0:3], r[:, 3:6], r[:, 6:9] = p1, p2 - p1, p3 - p1
    return r


def quads(seed):
    """a random quad scene of tests/scenes.py in which every triangle has a table: most of those scenes hold slivers or quads smaller than
    the rays' 0.01 offset, whose triangles have none (pt_sm_geom) -- a scene with one declines the table on the device, and here its cells,
    all-ones, would go without a ray of their own"""
    t, _ = scenes.random_quads(seed)
    assert 2 <= len(t) <= 64
    return t


def degenerate():
    t = _scene.load_model()[0].copy()
    t["p3"][7] = t["p2"][7]   # e2 = e1: no plane
    return t


def sixty_four():
    t = np.concatenate([_scene.load_model()[0], quads(105), quads(1007)])
    assert len(t) == 64
    return t


def far_cornell():
    """the box x 37.5, moved 80 away from the origin of coordinates: the plane-distance form's rounding is a tenth of H, near the builder's limit"""
    t = _scene.load_model()[0].copy()
    for f in ("p1", "p2", "p3"):
        t[f][:, :3] = t[f][:, :3] * np.float32(37.5) + np.array([3.0, -80.0, 11.0], np.float32)
    return t


SCENES = {"cornell": lambda: _scene.load_model()[0], "far_cornell": far_cornell, "quads_a": lambda: quads(105), "quads_b": lambda: quads(654),
          "degenerate": degenerate, "sixty_four": sixty_four}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("secmask") / "secondary_masks_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(HERE, "secondary_masks_check.cpp")])
    return exe


def run_check(exe, tmp_path, tris, mode="check", extra=()):
    path = str(tmp_path / "records.f32")
    records(tris).tofile(path)
    r = subprocess.run([exe, mode, path, str(len(tris)), str(SEED), str(CELLS), *extra], capture_output=True, text=True, timeout=120)
    words = r.stdout.split()
    return r, dict(zip(words[0::2], (int(w) for w in words[1::2])))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_accepted_pair_is_missing_from_its_cell(checker, tmp_path, name):
    tris = SCENES[name]()
    assert len(tris) <= 64
    r, c = run_check(checker, tmp_path, tris)
    print(name, len(tris), "triangles:", r.stdout.strip())
    assert c["cells"] >= 2000
    assert c["missing"] == 0, r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert c["accepted"] > 0 and c["rays"] > c["uncovered"], "the draws test nothing"
    assert c["skipped"] * 20 <= c["cells"], "%d of %d sampled cells had no ray of their own" % (c["skipped"], c["cells"])
    if name == "degenerate":
        assert c["skipped"] > 0, "the degenerate triangle's cells were not met"
