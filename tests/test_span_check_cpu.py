"""The shim's buffer checks (csrc/pt_span.h: fits, aligned, apart) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program with its own main (tests/span_check.cpp): built and run here, on the host, without a GPU and outside Python."""
import os
import subprocess

from conftest import ROOT


def test_span_checks_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "span_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "span_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "span_check: ok", r.stdout + r.stderr
