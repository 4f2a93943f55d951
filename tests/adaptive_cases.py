"""The inputs of tests/test_gpu_adaptive.py and what the restatement (tests/adaptive_oracle.py) says of them: one table, so that
tests/test_adaptive_cpu.py proves on exactly the scenes, sizes and rules the device runs that the adaptive loop reaches its edges.
TEST INFRASTRUCTURE."""
from __future__ import annotations

import os
import re

import numpy as np

import adaptive_oracle as ao
import direct_oracle as do
import moments_oracle as mom
import roulette_cases as rc
from conftest import ROOT
from scenes import edge_scene

# ---- the whole loop: name -> (scene, W, H, K, B, R, cap, mis, dict of render_adaptive's arguments) -------------------------------------
# Cornell plain and MIS, and the scene that takes the LBVH by itself; the tolerances are ones at which the lists shrink pass by pass
# and still leave pixels that run to max_samples (tests/test_adaptive_cpu.py asserts both)
_RULE = dict(min_samples=8, max_samples=40, frames_per_pass=4, floor=1e-2)
LOOPS = {
    "cornell_plain": ("cornell", 24, 16, 1, 6, 3, 0.95, False, dict(tolerance=0.2, **_RULE)),
    "cornell_mis": ("cornell", 24, 16, 1, 6, 3, 0.95, True, dict(tolerance=0.25, **_RULE)),
    "lbvh_mis": (rc.LBVH[0], 24, 16, 2, 6, 3, 0.95, True, dict(tolerance=0.35, **_RULE)),
}


def _loop(name):
    scene, W, H, K, B, R, cap, mis, kw = LOOPS[name]
    L = ao.loop(edge_scene(scene)[1], W, H, K, B, R, cap, mis=mis, **kw)
    return np.array(L.passes, np.int64), L.moments, L.counts, L.fb, np.array(L.finite)


def loop(name) -> ao.Loop:
    """the restated loop of a LOOPS case: computed once, shared, read-only"""
    passes, m, counts, fb, finite = do.once(_loop, name)
    return ao.Loop(tuple(int(n) for n in passes), m, counts, fb, bool(finite))


# ---- the rule on hand-made records ------------------------------------------------------------------------------------------------
RULE = ao.Rule(tol2=0.25, floor2=0.5, min_samples=4, max_samples=64)   # powers of two: the boundary record is exact


def hand_records():
    """(records, active bool, what) -- pt_pixel_moments records at the rule's edges under RULE and what the rule must say of each"""
    rows = []

    def rec(what, want, n, rejected, s, s2):
        rows.append((what, want, n, rejected, s, s2))

    rec("n = 0", True, 0, 0, 0.0, 0.0)
    rec("n = 1", True, 1, 0, 3.0, 9.0)
    rec("n >= min, variance 0", False, 8, 0, 8.0, 8.0)
    rec("sum2 - sum * mean negative", False, 8, 0, 8.0, 7.5)
    rec("taken >= max_samples with n < min", False, 2, 62, 1.0, 1.0)
    rec("rejected > 0, still short of min", True, 3, 5, 1.0, 1.0)
    rec("rejected > 0, noisy", True, 8, 3, 8.0, 800.0)
    # one channel with mean 1 and variance v, n = 8: b = v / 8, c = 1, tol2 * (c + floor2) = 0.375: v = 3 sits on the boundary
    # (sum = 8, sum2 = 8 + 7 v: all exact in binary64)
    rec("b == tol2 * (c + floor2) exactly", False, 8, 0, 8.0, 29.0)
    rec("b just above the boundary", True, 8, 0, 8.0, 29.0 + 2.0 ** -40)
    rec("a sum overflowed to infinity", False, 8, 0, np.inf, np.inf)
    rec("taken == max_samples - 1, noisy", True, 63, 0, 63.0, 6300.0)
    rec("taken == max_samples, noisy", False, 64, 0, 64.0, 6400.0)
    rec("n + rejected passes 2^32", False, 0xFFFFFFFF, 2, 1.0, 1e30)
    m = mom.zeros(len(rows))
    for i, (_, _, n, rejected, s, s2) in enumerate(rows):
        m["n"][i], m["rejected"][i] = n, rejected
        m["sum"][i] = (s, 0.0, 0.0)
        m["sum2"][i] = (s2, 0.0, 0.0)
    return m, np.array([r[1] for r in rows]), [r[0] for r in rows]


# ---- select alone -----------------------------------------------------------------------------------------------------------------
def scan_tile() -> int:
    """PT_LIGHT_SCAN_TILE of csrc/pt_kernels.h: the pixels a workgroup of the compaction owns"""
    text = open(os.path.join(ROOT, "oclpathtracer_amd", "csrc", "pt_kernels.h")).read()
    block, items = (int(re.search(r"^#define %s (\d+)\s*$" % k, text, re.M).group(1)) for k in ("PT_LIGHT_SCAN_BLOCK", "PT_LIGHT_SCAN_ITEMS"))
    return block * items


def select_sizes():
    t = scan_tile()
    return [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]


PATTERNS = ("none", "all", "every_other", "last_only", "seeded")


def select_records(pixels, pattern):
    """records of ``pixels`` pixels under RULE whose active set is the pattern's: an inactive record has converged (n = 8, variance
    0), an active one is one of three kinds in turn -- too few samples, noisy, noisy with rejected samples -- each with a frame number
    of its own; the hand-made records stand in front where they fit and the pattern permits"""
    rng = np.random.default_rng(pixels * 7 + PATTERNS.index(pattern))
    want = {"none": np.zeros(pixels, bool), "all": np.ones(pixels, bool), "every_other": np.arange(pixels) % 2 == 0,
            "last_only": np.arange(pixels) == pixels - 1, "seeded": rng.uniform(size=pixels) < 0.3}[pattern]
    m = mom.zeros(pixels)
    m["n"], m["sum"][:, 0], m["sum2"][:, 0] = 8, 8.0, 8.0
    a = np.flatnonzero(want)
    kind = np.arange(len(a)) % 3
    n = np.where(kind == 0, rng.integers(0, 4, len(a)), rng.integers(8, 40, len(a))).astype(np.uint32)
    m["n"][a] = n
    m["rejected"][a] = np.where(kind == 2, rng.integers(1, 9, len(a)), 0)
    m["sum"][a, 0] = n
    m["sum2"][a, 0] = n * 100.0
    if pattern == "seeded":
        hand, hand_active, _ = hand_records()
        k = min(len(hand), pixels)
        m[:k], want[:k] = hand[:k], hand_active[:k]
    return m, want
