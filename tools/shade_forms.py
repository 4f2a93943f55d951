#!/usr/bin/env python3
"""pt_shade's short forms against the literal operations, on the GPU (csrc/pt_kernels.hip, pt_shade_check_kernel):

    mode 1  pt_rsqrt_near1(x) against 1.0f / sqrtf(x)  for every binary32 of [1 - 2^-11, 1 + 2^-11]  (unit vectors)
    mode 3  pt_rcp_fast(x) against 1.0f / x            for every binary32 of [2^-60, 1e20]  (the guarded quotients' divisors)
    mode 2  pt_div, pt_div_by, pt_div_pair against "/" for 122 x 122 binade pairs (2^-61 .. 2^60: the window and the first
            binade outside on each side), 4096 significand pairs each

Usage: python tools/shade_forms.py      (about a second each)
"""
import struct
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import torch  # noqa: F401  (first: the shim binds to the HIP runtime torch loaded)

from oclpathtracer_amd import adl  # noqa: E402

BINADES, SIGS = 122, 4096


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def check(dev, mode, first, count):
    k = dev.getKernel("PtShimTest", "ShadeCheckKernel")
    assert k is not None
    out = adl.Buffer(dev, 8, np.uint64)
    try:
        out.write(np.zeros(8, np.uint64), 8)
        la = adl.Launcher(dev, k)
        la.setBuffers([adl.BufferInfo(out)])
        la.setConst(np.int32(mode))
        la.setConst(np.uint32(first))
        la.setConst(np.uint64(count))
        la.launch1D(1)
        res = np.empty(8, np.uint64)
        out.read(res, 8)
        dev.waitForCompletion()
    finally:
        out.release()
    return [int(v) for v in res]


def failing_range(res):
    lo, hi = ~res[7] & 0xFFFFFFFF, res[6]
    return "  failing operands between %#010x (%g) and %#010x (%g)" % (
        lo, struct.unpack("<f", struct.pack("<I", lo))[0], hi, struct.unpack("<f", struct.pack("<I", hi))[0])


def main():
    assert adl.init(adl.TYPE_HIP)
    dev = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    bad = 0
    for mode, what, lo, hi in ((1, "pt_rsqrt_near1(x) against 1.0f / sqrtf(x)", 1.0 - 2.0 ** -11, 1.0 + 2.0 ** -11), (3, "pt_rcp_fast(x) against 1.0f / x", 2.0 ** -60, 1e20)):
        t0 = time.time()
        res = check(dev, mode, bits(lo), bits(hi) - bits(lo) + 1)
        n = res[mode]
        print("mode %d: %s, every binary32 of [%.10g, %.10g] (%#010x .. %#010x): %d operands, %d mismatches (%.1f s)"
              % (mode, what, lo, hi, bits(lo), bits(hi), res[4], n, time.time() - t0))
        if n:
            print(failing_range(res))
        bad += n
    t0 = time.time()
    res = check(dev, 2, 20261018, BINADES * BINADES * SIGS)
    print("mode 2: pt_div, pt_div_by and pt_div_pair against \"/\", %d x %d binade pairs (2^-61 .. 2^60) x %d significand pairs: %d operand pairs, "
          "%d of them inside the window [2^-60, 2^60) of both operands, %d mismatches (%.1f s)" % (BINADES, BINADES, SIGS, res[4], res[5], res[2], time.time() - t0))
    if res[2]:
        print(failing_range(res))
    bad += res[2]
    adl.DeviceUtils.deallocate(dev)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    raise SystemExit(main())
