"""The continuous-batching scheduler's rules (csrc/sched.h) on a CPU: tests/native/sched_main.cpp,
a stand-alone program that includes only that header, built with a plain C++17 compiler (no ROCm
include path, no HIP header) under AddressSanitizer + UndefinedBehaviorSanitizer. It checks
hand-worked cases of prompt assembly, seed offsets, hard_min / sem_limit / step limit, the mixed
step's row budget, the decode plan, the window length, the head-rows rule, the token-progress
range and the run-ahead predicate, and the row-table invariants on random slot sets."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ (sanitizer runtimes) not present")
def test_sched_rules_under_asan_ubsan(tmp_path):
    exe = tmp_path / "sched_check"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "native", "sched_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "sched: ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
