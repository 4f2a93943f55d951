"""The masked search's pending-pair list, modelled on the host (tools/pair_list_model.cpp): a property of the candidate masks.

The model draws renderer-like rays on the Cornell box (seed 1, 61 000 rays, waves of 61), keeps every ray's mask and walks each form of
the search as the kernel does.  The form that ships builds ONE list per search with helper lanes (csrc/pt_kernels.hip:
pt_pair_list_build), after own steps down to PT_PAIR_TAIL_LANES lanes; the form it replaced ran a chunk per mask word, down to the
two-pass search's PT_TAIL_LANES.  The shipped form's list-building loop must run fewer iterations per search than the two chunks'
loops did -- 9.16 then, 6.9 at the most now."""
import os
import re
import subprocess

import pytest

from oclpathtracer_amd import scene as _scene
from test_secondary_masks_cpu import records
from test_secondary_masks_tight_cpu import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHIPPED = {0: "chunks", 1: "one_set", 2: "helpers"}


def shipped_form():
    """the form and the lanes at which its own steps stop, and the lanes at which the two-pass search's stop"""
    text = open(os.path.join(ROOT, "oclpathtracer_amd", "csrc", "pt_kernels.hip")).read()
    tail = int(re.search(r"^#define PT_TAIL_LANES (\d+)", text, re.M).group(1))
    own = int(re.search(r"^#define PT_PAIR_TAIL_LANES \(PT_TAIL_LANES < (\d+) \? PT_TAIL_LANES : \1\)", text, re.M).group(1))
    return SHIPPED[int(re.search(r"^#define PT_PAIR_LIST (\d+)", text, re.M).group(1))], min(own, tail), tail


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    d = tmp_path_factory.mktemp("pair_list_model")
    exe = str(d / "pair_list_model")
    subprocess.check_call([os.environ.get("CXX", "g++"), *FLAGS, "-o", exe, os.path.join(ROOT, "tools", "pair_list_model.cpp")])
    tris = _scene.load_model()[0]
    path = str(d / "records.f32")
    records(tris).tofile(path)

    def run(tail_lanes):
        r = subprocess.run([exe, path, str(len(tris)), "1", "61000", "61", str(tail_lanes)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        print(r.stdout.strip())
        out = {}
        for line in r.stdout.splitlines():
            w = line.split()
            if w[0] == "form":
                out[w[1]] = {w[i]: float(w[i + 1]) for i in range(2, len(w) - 1, 2)}
        return out
    return run


def test_the_shipped_form_builds_its_list_in_fewer_iterations_than_two_chunks(forms):
    name, own_lanes, tail_lanes = shipped_form()
    assert name != "chunks", "the masked search runs a chunk per word again"
    shipped, chunks = forms(own_lanes)[name]["list_iterations"], forms(tail_lanes)["chunks"]["list_iterations"]
    print("list iterations per search: %s %.2f, chunks %.2f" % (name, shipped, chunks))
    assert shipped < chunks
    assert shipped <= 6.9
