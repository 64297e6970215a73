"""Leveller timings: nothing here is gated, these are the baseline numbers -- there is no
earlier implementation to compare with.

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz), each
           with its own target, through one level_batch call: the HIP-event time of the launch triple
           (measure + gain + apply) and the call's wall time (copies included), medians after a warm-up;
  long     one 41 s utterance (656,000 samples);
  cpu      the same signals through the numpy restatement (tests/level_ref.py), one timed run each;
  share    the measure kernel's L * N multiply-adds per second of the triple's kernel time (an upper
           bound on the measure kernel's own time) against the f32 rate of a multiply and an add that
           are not fused: half of the 157.3 TFLOPS vector peak, 39.3 T multiply-adds per second.
Usage: level_bench.py [--out FILE.json] [--reps N] [--warmup N] [--no-cpu]"""
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

import level_ref  # noqa: E402
import rwkvtts  # noqa: E402
from rwkvtts import audio  # noqa: E402

B, N = 32, 512 * 320
N_LONG = 41 * 16000
PEAK_MADDS = 157.3e12 / 4.0  # unfused: two instructions per multiply-add, each at half the FMA peak's FLOP rate


def _speechlike(rng, n):
    """Harmonics of a wandering pitch under a slow envelope with pauses, plus a little noise."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * np.clip(np.sin(2 * np.pi * 3.1 * t) + 0.3, 0.0, None)
    x = x * (np.sin(2 * np.pi * 0.21 * t + rng.uniform(0, 6.28)) > -0.8)
    return (rng.uniform(0.02, 0.4) * x + 0.001 * rng.standard_normal(n)).astype(np.float32)


def timed(lv, signals, dbs, reps, warmup):
    for _ in range(warmup):
        lv.level_batch(signals, dbs)
    k, w = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = lv.level_batch(signals, dbs)
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(lv.kernel_ms())
    n = sum(x.size for x in signals)
    km = statistics.median(k)
    madds = float(lv.taps) * n
    return out, {"samples": n, "kernel_ms_median": round(km, 4), "kernel_ms_min": round(min(k), 4),
                 "kernel_ms_max": round(max(k), 4), "call_wall_ms_median": round(statistics.median(w), 3),
                 "measure_multiply_adds": madds, "multiply_adds_per_s_over_triple_time": round(madds / (km * 1e-3), 1),
                 "share_of_unfused_f32_peak": round(madds / (km * 1e-3) / PEAK_MADDS, 4)}


def cpu_row(signals, dbs, outs):
    t0 = time.perf_counter()
    ref = [level_ref.level(x, db) for x, db in zip(signals, dbs)]
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
    lv = audio.Leveller(device=0)
    res = {"batch_shape": f"{B} x {N} samples @ 16 kHz", "long_shape": f"1 x {N_LONG} samples @ 16 kHz", "block": lv.block,
           "taps": lv.taps, "lookahead": lv.lookahead, "reps": a.reps, "warmup": a.warmup,
           "peak_unfused_f32_multiply_adds_per_s": PEAK_MADDS, "build_id": rwkvtts._ffi.build_id()}
    batch = [_speechlike(rng, N) for _ in range(B)]
    dbs = [-23.0 + 7.0 * (i % 2) - 0.1 * i for i in range(B)]
    outs, res["batch"] = timed(lv, batch, dbs, a.reps, a.warmup)
    long_ = [_speechlike(rng, N_LONG)]
    outs_long, res["long"] = timed(lv, long_, [-16.0], a.reps, a.warmup)
    lv.close()
    if not a.no_cpu:
        res["batch"]["cpu"] = cpu_row(batch, dbs, outs)
        res["long"]["cpu"] = cpu_row(long_, [-16.0], outs_long)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
