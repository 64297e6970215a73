"""The pitch shifter's host-only rules (csrc/pitch_plan.h) on a CPU: tests/native/pitch_plan_main.cpp,
a stand-alone program that includes only that header, built with a plain C++17 compiler (no ROCm
include path, no HIP header) under AddressSanitizer + UndefinedBehaviorSanitizer. It checks the
ranges of a desc, the table's length (filled into a buffer of exactly that length), the plan's
formulas and a window's refusals, and, against both walks simulated over random period arrays and
random cuts, that every carried state passes the state check, that the mark lists fit the sizes
the launches reserve, and that every frame and sample a window needs is kept and known."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ (sanitizer runtimes) not present")
def test_pitch_plan_rules_under_asan_ubsan(tmp_path):
    exe = tmp_path / "pitch_plan_check"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "native", "pitch_plan_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "pitch_plan: ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
