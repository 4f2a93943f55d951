"""The shape of the secondary rays' table (csrc/pt_secmask.h: PT_SM_T tiles per edge, PT_SM_C direction cells per edge), on the host.

tools/secmask_candidates.cpp, the estimator of profiles/*/candidates.txt, is built twice: with the header's own PT_SM_T and PT_SM_C (the
shape that ships) and with -DPT_SM_T=12 -DPT_SM_C=8 (the shape this one replaced).  Both read the Cornell box at the same arguments --
seed 20261021, 60 000 rays, 150 dense cells of 2 000 rays.  The shipped shape must leave no ray uncovered, hold every pair a dense-sample
ray is accepted for, and bring pass 2 at least 0.4 candidates per ray fewer than the earlier shape: every finalist of the sweep that chose
it read 0.45 or more below, and a shape that brings less is not worth its bytes.  Both tables are supersets by the same proof, so the
earlier shape is held to the same two zeros.  Nothing here assumes an even C, or 6 C^2 a multiple of the wave."""
import os
import re
import subprocess

import pytest

from oclpathtracer_amd import scene as _scene
from test_secondary_masks_cpu import records
from test_secondary_masks_tight_cpu import FLAGS, SEED, counters

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PARENT_SHAPE = (12, 8)
GAIN = 0.4
ARGS = [str(SEED), "60000", "150", "2000"]


def header_shape():
    text = open(os.path.join(ROOT, "oclpathtracer_amd", "csrc", "pt_secmask.h")).read()
    return tuple(int(re.search(r"^#define %s (\d+)$" % name, text, re.M).group(1)) for name in ("PT_SM_T", "PT_SM_C"))


@pytest.fixture(scope="module")
def readings(tmp_path_factory):
    """the estimator's counters for the shipped shape and for the earlier one: {"shipped": .., "parent": ..}"""
    d = tmp_path_factory.mktemp("secmask_shape")
    source = os.path.join(ROOT, "tools", "secmask_candidates.cpp")
    tris = _scene.load_model()[0]
    path = str(d / "records.f32")
    records(tris).tofile(path)
    out = {}
    for name, defs in (("shipped", []), ("parent", ["-DPT_SM_T=%d" % PARENT_SHAPE[0], "-DPT_SM_C=%d" % PARENT_SHAPE[1]])):
        exe = str(d / ("secmask_candidates_" + name))
        subprocess.check_call([os.environ.get("CXX", "g++"), *FLAGS, *defs, "-o", exe, source])
        r = subprocess.run([exe, path, str(len(tris)), *ARGS], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        print(name, header_shape() if name == "shipped" else PARENT_SHAPE, r.stdout.strip())
        out[name] = counters(r.stdout)
    return out


@pytest.mark.parametrize("name", ["shipped", "parent"])
def test_no_ray_is_uncovered_and_no_accepted_pair_is_outside(readings, name):
    c = readings[name]
    assert c["uncovered"] == 0, "%s: %d rays of 60 000 have no cell" % (name, c["uncovered"])
    assert c["outside"] == 0, "%s: a dense-sample ray's accepted pair is outside the table" % name
    assert 0.9 < c["accepted"] < 1.1, "the rays are not the renderer's: the reference accepts about one pair per ray"
    assert c["union"] <= c["union_table"] <= c["candidates"] + 1.0
    assert c["candidates"] >= c["accepted"]


def test_the_shipped_shape_brings_fewer_candidates_than_the_one_it_replaced(readings):
    got, was = readings["shipped"]["candidates"], readings["parent"]["candidates"]
    print("candidates per ray: shipped shape %s %.4f, T = %d C = %d %.4f" % (header_shape(), got, *PARENT_SHAPE, was))
    assert 3.4 < was < 3.6, "T = 12, C = 8 read 3.5186 at these arguments, not %.4f: the estimator or the builder changed" % was
    assert got <= was - GAIN, "%.4f candidates per ray, the earlier shape's %.4f less %.1f is the bound" % (got, was, GAIN)


def test_the_largest_table_keeps_32_bit_offsets():
    T, C = header_shape()
    head = 64 * 48
    assert head + 64 * T * T * 6 * C * C * 8 < 1 << 32, "an entry's byte offset (pt_trace_body, pt_secondary_mask_kernel) no longer fits 32 bits"
    assert C <= 16, "pt_sm_classify's rounding bound is derived for C <= 16"
