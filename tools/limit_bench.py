"""Limiter timings, modelled on highband_bench.py: nothing here is gated. One process
times, in alternating repetitions, on speech-like signals resampled to 48 kHz and scaled so that their
peaks pass the ceiling:

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz, 491,520
           each at 48 kHz): one limit_batch call at -1 dB (the HIP-event time of k_limit), medians after
           a warm-up, with min and max; beside the vocoder's 51.8 ms for the same batch;
  long     one 41 s utterance (1,968,000 samples at 48 kHz), the same call;
  quiet    the batch scaled under the ceiling: every workgroup takes the copy path;
  numpy    the contract's restatement (tests/limit_ref.py) on the 41 s utterance, once, wall time.
Bytes per sample is 8 (one f32 read, one written): the rate each time implies is printed beside it.
Usage: limit_bench.py [--out FILE.json] [--reps N] [--warmup N]"""
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

import limit_ref  # noqa: E402
from pitch_bench import B, N, N_LONG, VOCODER_MS, _speechlike  # noqa: E402
from rwkvtts import audio  # noqa: E402

LIMIT_DB = -1.0


def stats(v, samples):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "gb_per_s_at_8_bytes_per_sample": round(8.0 * samples / (med * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    lim = audio.Limiter(device=0)
    rs = audio.Resampler(16000, 48000, device=0, align="zero")
    c = float(lim.ceiling(LIMIT_DB))

    def at48k(xs, peak):  # resampled, then scaled so that the largest sample is `peak` times the ceiling
        return [(y * (peak * c / np.max(np.abs(y)))).astype(np.float32) for y in rs.resample_batch(xs)]

    batch = [_speechlike(rng, N).astype(np.float32) for _ in range(B)]
    cases = {"batch": at48k(batch, 1.5), "long": at48k([_speechlike(rng, N_LONG).astype(np.float32)], 1.5),
             "quiet": at48k(batch, 0.5)}
    t = {k: [] for k in cases}
    bound = {}
    for r in range(a.warmup + a.reps):
        for k, xs in cases.items():  # alternating: every round runs each case once, in order
            ys = lim.limit_batch(xs, [LIMIT_DB] * len(xs))
            if r >= a.warmup:
                t[k].append(lim.kernel_ms())
            bound[k] = float(np.mean([np.mean(y != x) for x, y in zip(xs, ys)]))
    out = {"reps": a.reps, "warmup": a.warmup, "limit_db": LIMIT_DB, "vocoder_ms_same_batch": VOCODER_MS, "cases": {}}
    for k, xs in cases.items():
        total = int(sum(x.size for x in xs))
        out["cases"][k] = {"signals": len(xs), "samples_each": int(xs[0].size), "share_of_samples_changed": round(bound[k], 5),
                           "limit_kernel": stats(t[k], total)}
    out["cases"]["batch"]["limit_over_vocoder"] = round(out["cases"]["batch"]["limit_kernel"]["median_ms"] / VOCODER_MS, 5)
    x = cases["long"][0]
    t0 = time.perf_counter()
    ref = limit_ref.limit(x, LIMIT_DB, tab=lim.table)
    out["numpy_contract_41s_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    y = lim.limit(x, LIMIT_DB)
    out["long_is_bitwise_the_contract"] = bool(np.array_equal(ref.view(np.uint32), y.view(np.uint32)))
    out["long_peak_over_ceiling"] = {"in": round(float(np.max(np.abs(x))) / c, 4), "out": round(float(np.max(np.abs(y))) / c, 6)}
    for s in (lim, rs):
        s.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
