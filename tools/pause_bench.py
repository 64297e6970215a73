"""Pause-stage timings: nothing here is gated, these are the baseline numbers -- there
is no earlier implementation to compare with.

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz), each
           with its own cap, through one shape_samples_batch call: the HIP-event time of the launch
           triple (flags + plan + gather) and the call's wall time (copies and the extra read-back of
           the counts included), medians after a warm-up;
  long     one 41 s utterance (656,000 samples, 4100 blocks): the plan kernel's one workgroup per
           signal is the exposed part here;
  cpu      the same signals through the numpy restatement (tests/pause_ref.py), one timed run each;
  beside   the vocoder's time for the same batch, as DESIGN.md records it (51.8 ms), and the bytes the
           triple moves (each input sample read by the flags and, where kept, by the gather, each
           output written once) per second of kernel time.
Usage: pause_bench.py [--out FILE.json] [--reps N] [--warmup N] [--no-cpu]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwkv-tts-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import pause_ref  # noqa: E402
import rwkvtts  # noqa: E402
from rwkvtts import audio  # noqa: E402

B, N = 32, 512 * 320
N_LONG = 41 * 16000
VOCODER_MS = 51.8  # the vocoder's kernel time for the same batch


def _speechlike(rng, n):
    """Harmonics of a wandering pitch under a slow envelope with pauses of up to a second and more,
    plus noise under the threshold."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * np.clip(np.sin(2 * np.pi * 3.1 * t) + 0.3, 0.0, None)
    x = x * (np.sin(2 * np.pi * 0.21 * t + rng.uniform(0, 6.28)) > 0.2)
    return (rng.uniform(0.05, 0.4) * x + 0.001 * rng.standard_normal(n)).astype(np.float32)


def timed(ps, signals, caps, reps, warmup):
    for _ in range(warmup):
        ps.shape_samples_batch(signals, caps)
    k, w = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ps.shape_samples_batch(signals, caps)
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(ps.kernel_ms())
    n, n_out = sum(x.size for x in signals), sum(y.size for y in out)
    km = statistics.median(k)
    moved = 4.0 * (n + 2 * n_out)
    return out, {"samples": n, "samples_out": n_out, "cuts": int(sum(ps.cuts)), "kernel_ms_median": round(km, 4),
                 "kernel_ms_min": round(min(k), 4), "kernel_ms_max": round(max(k), 4),
                 "call_wall_ms_median": round(statistics.median(w), 3), "bytes_moved": moved,
                 "gb_per_s_over_triple_time": round(moved / (km * 1e-3) / 1e9, 1)}


def cpu_row(ps, signals, caps, outs):
    t0 = time.perf_counter()
    ref = [pause_ref.shape(x, m, ps.block, ps.hang, ps.fade, ps.threshold)[0] for x, m in zip(signals, caps)]
    ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ref, outs))
    return {"numpy_restatement_ms": round(ms, 1), "bitwise_equal_to_gpu": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ps = audio.PauseShaper(device=0)
    res = {"batch_shape": f"{B} x {N} samples @ 16 kHz", "long_shape": f"1 x {N_LONG} samples @ 16 kHz", "block": ps.block,
           "hang": ps.hang, "fade": ps.fade, "threshold": ps.threshold, "reps": a.reps, "warmup": a.warmup,
           "vocoder_ms_same_batch": VOCODER_MS, "build_id": rwkvtts._ffi.build_id()}
    batch = [_speechlike(rng, N) for _ in range(B)]
    caps = [ps.samples(200 + 25 * i) for i in range(B)]
    outs, res["batch"] = timed(ps, batch, caps, a.reps, a.warmup)
    res["batch"]["share_of_vocoder_time"] = round(res["batch"]["kernel_ms_median"] / VOCODER_MS, 5)
    long_ = [_speechlike(rng, N_LONG)]
    outs_long, res["long"] = timed(ps, long_, [ps.samples(300)], a.reps, a.warmup)
    ps.close()
    if not a.no_cpu:
        res["batch"]["cpu"] = cpu_row(ps, batch, caps, outs)
        res["long"]["cpu"] = cpu_row(ps, long_, [300 * 16], outs_long)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
