"""csrc/manager.cpp's streaming entry points under ThreadSanitizer on the CPU: compiled unchanged
against the stub engine of tests/native/stream/engine.h (it delivers partial tokens from the engine's
owner thread, and serves greedy = 1 requests the old way, with no progress), driven by
tests/native/stream/manager_stream_tsan_main.cpp as one stand-alone program: threads running
submit_stream, submit, wait_tokens and wait at once, a request that fails half-way, destroy with
blocked wait_tokens callers. What wait_tokens hands out is always a growing prefix of the final
result, and a request served without progress still ends with all its tokens."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ (TSan runtime) not present")
def test_manager_streaming_under_tsan(tmp_path):
    src = os.path.join(ROOT, "rwkv-tts-rs_amd", "csrc", "manager.cpp")
    stub = os.path.join(ROOT, "tests", "native", "stream")
    rccl = os.path.join(ROOT, "tests", "native", "stub")  # <rccl/rccl.h>: the declarations only
    # manager.cpp includes "engine.h" from its own directory: build a copy beside the stub engine
    shutil.copy(src, tmp_path / "manager.cpp")
    eh = open(os.path.join(stub, "engine.h")).read().replace('"../../../include/rwkvtts.h"', '"rwkvtts.h"')
    (tmp_path / "engine.h").write_text(eh)
    main = open(os.path.join(stub, "manager_stream_tsan_main.cpp")).read()
    (tmp_path / "main.cpp").write_text(main)
    exe = tmp_path / "manager_stream_tsan"
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-Wno-enum-compare",
                           "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"), "-I", rccl, "-o", str(exe),
                           str(tmp_path / "main.cpp"), str(tmp_path / "manager.cpp"), "-ldl", "-lpthread"])
    env = dict(os.environ, RWKVTTS_MANAGER_NO_RCCL="1", TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    env.pop("STUB_FAIL_SEED", None)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "manager_stream_tsan: ok" in out.stdout, (out.stdout[-2000:], out.stderr[-6000:])
    assert "ThreadSanitizer" not in out.stderr, out.stderr[-6000:]
