"""CPU witness of the near-1 form of 1 / sqrt(x) that pt_shade's normalisations of unit vectors take (csrc/pt_device_math.h,
pt_rsqrt_near1): six fused multiply-adds, no transcendental, so the same bits on any IEEE machine.  tests/shade_near1.c restates
it in C (compiled without contraction); EVERY binary32 of the window 1 +- 2^-11 is compared with 1.0f / sqrtf(x).  The GPU
tier runs the device function over the same window (tests/test_gpu_shade_forms.py, mode 1)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


@pytest.fixture(scope="module")
def near1(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path_factory.mktemp("near1") / "shade_near1")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(HERE, "shade_near1.c"), "-lm"])

    def run(lo, hi, plain=0):
        n, bad, first = subprocess.check_output([exe, _bits(lo), _bits(hi), str(plain)]).decode().split()
        return int(n), int(bad), int(first, 16)
    return run


def test_every_binary32_of_the_window_gets_both_roundings(near1):
    n, bad, _ = near1(1.0 - 2.0 ** -11, 1.0 + 2.0 ** -11)
    assert n == (1 << 13) + (1 << 12) + 1     # 2^13 floats below 1 (spacing 2^-24), 2^12 above (2^-23), and 1
    assert bad == 0


def test_the_test_can_fail(near1):
    """the same sequence with 1/2, 1/2 and 1 for its constants misses 1 - 2^-24 and 1 - 2^-23, and the window is not generous:
    twice as wide, values fail on both sides"""
    n, bad, first = near1(1.0 - 2.0 ** -11, 1.0 + 2.0 ** -11, plain=1)
    assert bad == 2 and first == int(_bits(1.0 - 2.0 ** -23), 16)
    assert near1(1.0 - 2.0 ** -10, np.nextafter(np.float32(1.0 - 2.0 ** -11), np.float32(0.0)))[1] > 0
    assert near1(np.nextafter(np.float32(1.0 + 2.0 ** -11), np.float32(2.0)), 1.0 + 2.0 ** -10)[1] > 0
