"""CPU witness of the exponent ranges of the GGX branch's guarded quotients (csrc/pt_device_math.h: pt_div, pt_div_by, pt_div_pair):
tests/shade_quotients.c restates them with the correctly rounded reciprocal where the device runs pt_rcp_fast, and compares them
with "/" over every pair of binades 2^-61 .. 2^60 -- the window [2^-60, 2^60) of both operands and the first binade outside on
each side -- with all-zeros and all-ones significands, a +0 numerator and arbitrary significands.  The device functions themselves,
v_rcp_f32 included, are compared the same way on the GPU (tests/test_gpu_shade_forms.py, modes 2 and 3)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_guarded_quotients_over_every_pair_of_binades(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "shade_quotients")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(HERE, "shade_quotients.c"), "-lm"])
    nsig = 256
    n, inside, bad = (int(v) for v in subprocess.check_output([exe, str(nsig)]).decode().split())
    assert n == 122 * 122 * nsig
    assert inside == 120 * 120 * (nsig - 1)      # (the +0 numerator is outside the window)
    assert bad == 0
