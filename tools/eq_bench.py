"""Equaliser timings, modelled on limit_bench.py: nothing here is gated. One process times,
in alternating repetitions, on speech-like 16 kHz signals, at N = 64, 1024 and 4096 taps passed in directly
(uniform random taps: the kernel's time does not depend on their values):

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples): one eq_batch call (the
           HIP-event time of k_eq), medians after a warm-up, with min and max; beside the vocoder's 51.8 ms
           for the same batch;
  long     one 41 s utterance (656,000 samples), the same call;
  numpy    the contract's restatement (tests/eq_ref.py) on the 41 s utterance, once per N, wall time.
A tap is one multiply and one add: the rate each time implies is printed beside it, 2 N operations a sample.
Usage: eq_bench.py [--out FILE.json] [--reps N] [--warmup N]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwkv-tts-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import eq_ref  # noqa: E402
from pitch_bench import B, N, N_LONG, VOCODER_MS, _speechlike  # noqa: E402
from rwkvtts import audio  # noqa: E402

TAPS = (64, 1024, 4096)


def stats(v, samples, n_taps):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "tflops_at_2_ops_per_tap": round(2.0 * n_taps * samples / (med * 1e-3) / 1e12, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    eq = audio.Equaliser(device=0)
    signals = {"batch": [_speechlike(rng, N).astype(np.float32) for _ in range(B)],
               "long": [_speechlike(rng, N_LONG).astype(np.float32)]}
    taps = {n: rng.uniform(-1.0, 1.0, n).astype(np.float32) / np.float32(n) for n in TAPS}
    t = {(k, n): [] for k in signals for n in TAPS}
    for r in range(a.warmup + a.reps):
        for key in t:  # alternating: every round runs each case once, in order
            eq.eq_batch(signals[key[0]], [0] * len(signals[key[0]]), table=[taps[key[1]]])
            if r >= a.warmup:
                t[key].append(eq.kernel_ms())
    out = {"reps": a.reps, "warmup": a.warmup, "vocoder_ms_same_batch": VOCODER_MS, "cases": {}}
    for (k, n), v in t.items():
        xs = signals[k]
        case = out["cases"].setdefault(k, {"signals": len(xs), "samples_each": int(xs[0].size), "eq_kernel": {}})
        case["eq_kernel"][str(n)] = stats(v, int(sum(x.size for x in xs)), n)
        if k == "batch":
            case["eq_kernel"][str(n)]["eq_over_vocoder"] = round(statistics.median(v) / VOCODER_MS, 4)
    x = signals["long"][0]
    out["numpy_contract_41s_wall_ms"], out["long_is_bitwise_the_contract"] = {}, {}
    for n in TAPS:
        t0 = time.perf_counter()
        ref = eq_ref.fir(x, taps[n])
        out["numpy_contract_41s_wall_ms"][str(n)] = round((time.perf_counter() - t0) * 1e3, 1)
        y = eq.eq_batch([x], [0], table=[taps[n]])[0]
        out["long_is_bitwise_the_contract"][str(n)] = bool(np.array_equal(ref.view(np.uint32), y.view(np.uint32)))
    eq.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
