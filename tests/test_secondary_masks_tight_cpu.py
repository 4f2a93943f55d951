"""The refined builder of the secondary rays' masks (csrc/pt_secmask.h: adaptive boxes and the separating plane), on the host.

DENSE CONTAINMENT.  tests/secondary_masks_tight_check.cpp fills a seeded sample of cells with rays -- origins over the whole tile and the
whole +-H slab, on tile edges and at +-H; direction ratios over the whole direction cell and on its edges -- classifies each with
pt_sm_classify and requires that no pair the reference's binary32 test accepts is missing from the mask of the cell the ray lands in.
The separating plane proves that NO ray of a box passes all five conditions at once; an error in it removes a triangle that only rays
of one corner of the cell reach, which the 240 boundary rays per cell of tests/test_secondary_masks_cpu.py were not drawn to find.
At most 5 % of the sampled cells may go without a ray of their own (that test's cap).

TIGHTNESS.  tools/secmask_candidates.cpp, the estimator of profiles/tight_masks/candidates.txt, draws renderer-like rays on the Cornell box
with a fixed seed; the candidates per ray of the table as shipped must be at most 3.6 (the fixed-grid builder read 4.25 to 4.52, and a
builder that keeps everything reads 36).  The estimator's own dense-sample union of the visited cells must lie inside the table too."""
import os
import subprocess

import pytest

from oclpathtracer_amd import scene as _scene
from test_secondary_masks_cpu import far_cornell, quads, records, sixty_four

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 20261021
CELLS = 300
RAYS = 3000
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]
CANDIDATES_BOUND = 3.6


def one_quad():
    """the floor of the box alone: two triangles, each other's only target"""
    return _scene.load_model()[0][:2].copy()


def thirty_three():
    """33 triangles of the box: the second mask word holds exactly one bit"""
    return _scene.load_model()[0][:33].copy()


SCENES = {"cornell": lambda: _scene.load_model()[0], "far_cornell": far_cornell, "quads_105": lambda: quads(105), "quads_1007": lambda: quads(1007),
          "sixty_four": sixty_four, "one_quad": one_quad, "thirty_three": thirty_three}


def build(tmp, source, name):
    exe = str(tmp / name)
    subprocess.check_call([os.environ.get("CXX", "g++"), *FLAGS, "-o", exe, source])
    return exe


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    return build(tmp_path_factory.mktemp("secmask_tight"), os.path.join(HERE, "secondary_masks_tight_check.cpp"), "secondary_masks_tight_check")


@pytest.fixture(scope="module")
def estimator(tmp_path_factory):
    return build(tmp_path_factory.mktemp("secmask_est"), os.path.join(ROOT, "tools", "secmask_candidates.cpp"), "secmask_candidates")


def counters(stdout):
    """'name value name value ..' up to the first word that has no number after it"""
    w, out, i = stdout.split(), {}, 0
    while i + 1 < len(w):
        try:
            out[w[i]] = float(w[i + 1])
        except ValueError:
            break
        i += 2
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_dense_rays_of_a_cell_find_every_accepted_pair_in_its_mask(dense, tmp_path, name):
    tris = SCENES[name]()
    assert {"one_quad": 2, "thirty_three": 33, "sixty_four": 64}.get(name, len(tris)) == len(tris)
    path = str(tmp_path / "records.f32")
    records(tris).tofile(path)
    r = subprocess.run([dense, path, str(len(tris)), str(SEED), str(CELLS), str(RAYS)], capture_output=True, text=True, timeout=300)
    c = counters(r.stdout)
    print(name, len(tris), "triangles:", r.stdout.strip())
    assert c["cells"] == CELLS and c["rays"] == CELLS * RAYS
    assert c["missing"] == 0, r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert c["accepted"] > 0 and c["own"] > 0, "the draws test nothing"
    assert c["skipped"] * 20 <= c["cells"], "%d of %d sampled cells had no ray of their own" % (c["skipped"], c["cells"])
    if len(tris) > 2:
        assert c["kept"] < (c["rays"] - c["uncovered"]) * len(tris), "every mask keeps every triangle"


def test_the_cornell_box_brings_at_most_the_stated_candidates_per_ray(estimator, tmp_path):
    tris = _scene.load_model()[0]
    path = str(tmp_path / "records.f32")
    records(tris).tofile(path)
    r = subprocess.run([estimator, path, str(len(tris)), str(SEED), "60000", "150", "2000"], capture_output=True, text=True, timeout=300)
    c = counters(r.stdout)
    print(r.stdout.strip())
    assert r.returncode == 0 and c["outside"] == 0, "a dense-sample ray's accepted pair is outside the table: " + r.stdout + r.stderr
    assert c["uncovered"] == 0
    assert 0.9 < c["accepted"] < 1.1, "the rays are not the renderer's: the reference accepts about one pair per ray"
    assert c["union"] <= c["union_table"] <= c["candidates"] + 1.0
    assert c["candidates"] <= CANDIDATES_BOUND, "%.3f candidates per ray, the bound is %.1f" % (c["candidates"], CANDIDATES_BOUND)
    assert c["candidates"] >= c["accepted"]
