"""The request extension block and Mirostat through the scheduler's rules (csrc/sched.h) on a CPU:
tests/native/sched_miro_main.cpp, built like tests/native/sched_penalty_main.cpp (plain C++17, no
HIP header, AddressSanitizer + UndefinedBehaviorSanitizer). It checks every rejection of validate()
(each range edge on both sides, non-finite values, unknown bits, greedy, semantic_sampling), a short
struct_size (heap blocks of exactly that size: a read past one is an ASan report), that no block and
a block that sets nothing give the parent's admission byte for byte, the plan flag in decode_plan
and mixed_plan, and that normal, zero-shot and pinned admissions carry the block with mu = 2 tau."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ (sanitizer runtimes) not present")
def test_sched_miro_rules_under_asan_ubsan(tmp_path):
    exe = tmp_path / "sched_miro_check"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "sched_miro_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "sched miro: ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
