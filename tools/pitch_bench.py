"""Pitch-shifter timings: nothing here is gated, these are the baseline numbers -- there
is no earlier implementation to compare with. The yardstick is the vocoder's 51.8 ms for the same
batch.

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz), all at
           +4 semitones, through one shift_batch call: the HIP-event time of the launch triple (period +
           marks + synthesis), of the marks kernel alone (the serial walk, one wave per signal) and the
           call's wall time (copies included), medians after a warm-up;
  long     one 41 s utterance (656,000 samples): the walk is one wave's serial work here;
  cpu      the first batch signal and the long one through the numpy restatement (tests/pitch_ref.py),
           one timed run each, compared bit for bit;
  share    the period kernel's frames x lags x Wc steps, seven unfused f32 operations each, per second
           of the triple's kernel time (an upper bound on the period kernel's own time) against half
           of the 157.3 TFLOPS vector peak (no fused multiply-add anywhere in the contract).
Usage: pitch_bench.py [--out FILE.json] [--reps N] [--warmup N] [--no-cpu]"""
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

import pitch_ref  # noqa: E402
import rwkvtts  # noqa: E402
from rwkvtts import audio  # noqa: E402

B, N = 32, 512 * 320
N_LONG = 41 * 16000
SEMITONES = 4.0
VOCODER_MS = 51.8  # the same batch through the vocoder
PEAK_OPS = 157.3e12 / 2.0  # unfused f32 operations per second: half the FMA peak's FLOP rate


def _speechlike(rng, n):
    """Harmonics of a wandering pitch under a slow envelope with pauses, plus a little noise."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * np.clip(np.sin(2 * np.pi * 3.1 * t) + 0.3, 0.0, None)
    x = x * (np.sin(2 * np.pi * 0.21 * t + rng.uniform(0, 6.28)) > -0.8)
    return (rng.uniform(0.02, 0.4) * x + 0.001 * rng.standard_normal(n)).astype(np.float32)


def timed(ps, signals, reps, warmup):
    semis = [SEMITONES] * len(signals)
    for _ in range(warmup):
        ps.shift_batch(signals, semis)
    k, m, w = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ps.shift_batch(signals, semis)
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(ps.kernel_ms())
        m.append(ps.walk_ms())
    n = sum(x.size for x in signals)
    km = statistics.median(k)
    frames = sum((x.size + 2 * ps.lag_max - 1) // ps.hop + 1 for x in signals)
    ops = 7.0 * frames * (ps.lag_max - ps.lag_min + 3) * ps.window
    return out, {"samples": n, "kernel_ms_median": round(km, 4), "kernel_ms_min": round(min(k), 4),
                 "kernel_ms_max": round(max(k), 4), "walk_ms_median": round(statistics.median(m), 4),
                 "walk_ms_min": round(min(m), 4), "walk_ms_max": round(max(m), 4),
                 "call_wall_ms_median": round(statistics.median(w), 3), "period_f32_ops": ops,
                 "share_of_unfused_f32_peak": round(ops / (km * 1e-3) / PEAK_OPS, 4),
                 "kernel_ms_over_vocoder_ms": round(km / VOCODER_MS, 4)}


def cpu_row(x, out):
    t0 = time.perf_counter()
    y, _, _, per, a, pairs = pitch_ref.window(x, 0, True, audio.pitch_factor(SEMITONES), 0, 0, 0, x.size, want_marks=True)
    ms = (time.perf_counter() - t0) * 1e3
    return {"numpy_restatement_ms": round(ms, 1), "bitwise_equal_to_gpu": bool(np.array_equal(y.view(np.uint32), out.view(np.uint32))),
            "voiced_frames": int(np.count_nonzero(per)), "frames": int(per.size), "analysis_marks": len(a),
            "synthesis_marks": len(pairs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ps = audio.PitchShifter(device=0)
    res = {"batch_shape": f"{B} x {N} samples @ 16 kHz", "long_shape": f"1 x {N_LONG} samples @ 16 kHz", "semitones": SEMITONES,
           "hop": ps.hop, "window": ps.window, "lag_min": ps.lag_min, "lag_max": ps.lag_max, "unvoiced": ps.unvoiced,
           "reps": a.reps, "warmup": a.warmup, "vocoder_ms_same_batch": VOCODER_MS,
           "peak_unfused_f32_ops_per_s": PEAK_OPS, "build_id": rwkvtts._ffi.build_id()}
    batch = [_speechlike(rng, N) for _ in range(B)]
    outs, res["batch"] = timed(ps, batch, a.reps, a.warmup)
    long_ = [_speechlike(rng, N_LONG)]
    outs_long, res["long"] = timed(ps, long_, a.reps, a.warmup)
    ps.close()
    if not a.no_cpu:
        res["batch"]["cpu_first_signal"] = cpu_row(batch[0], outs[0])
        res["long"]["cpu"] = cpu_row(long_[0], outs_long[0])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
