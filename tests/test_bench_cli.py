"""bench.py's command line and output dump, as far as they go without a GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_writes_float_arrays(tmp_path):
    rs = np.random.RandomState(3)
    out = [(rs.randint(0, 4096, 32).tolist(), rs.randint(0, 8192, 5).tolist()) for _ in range(3)]
    pcm = [rs.randn(5 * 320).astype(np.float32) for _ in range(3)]
    d = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(d), out, pcm)
    assert sorted(os.listdir(d)) == ["global_tokens.npy", "pcm.npy", "semantic_tokens.npy"]
    g, s, p = (np.load(d / f"{n}.npy") for n in ("global_tokens", "semantic_tokens", "pcm"))
    assert g.dtype == np.float64 and g.shape == (3, 32) and g.tolist() == [x for x, _ in out]
    assert s.dtype == np.float64 and s.shape == (3, 5) and s.tolist() == [x for _, x in out]
    assert p.dtype == np.float32 and p.shape == (3, 1600) and np.array_equal(p, np.stack(pcm))


def test_options_present_and_steps_checked():
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *a],  # noqa: E731
                                    capture_output=True, text=True, timeout=60)
    h = run("--help")
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs DIR" in h.stdout
    z = run("--gpus", "1", "--steps", "0")
    assert z.returncode == 2 and "--steps must be at least 1" in z.stderr
