"""Noise-reduction timings, modelled on limit_bench.py: nothing here is gated. One process
times, in alternating repetitions, on speech-like 16 kHz signals at denoise = 12:

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples): one denoise_batch call
           (the HIP-event time of the launch triple k_dn_analyse, k_dn_gain, k_dn_synth), medians after a
           warm-up, with min and max; beside the vocoder's 51.8 ms for the same batch;
  long     one 41 s utterance (656,000 samples), the same call;
  numpy    the contract's restatement (tests/denoise_ref.py) on the 41 s utterance, once, wall time.
Usage: denoise_bench.py [--out FILE.json] [--reps N] [--warmup N]"""
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

import denoise_ref  # noqa: E402
from pitch_bench import B, N, N_LONG, VOCODER_MS, _speechlike  # noqa: E402
from rwkvtts import audio  # noqa: E402

DEPTH = 12.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    dn = audio.Denoiser(device=0)
    signals = {"batch": [_speechlike(rng, N).astype(np.float32) for _ in range(B)],
               "long": [_speechlike(rng, N_LONG).astype(np.float32)]}
    t = {k: [] for k in signals}
    for r in range(a.warmup + a.reps):
        for key, xs in signals.items():  # alternating: every round runs each case once, in order
            dn.denoise_batch(xs, [DEPTH] * len(xs))
            if r >= a.warmup:
                t[key].append(dn.kernel_ms())
    out = {"reps": a.reps, "warmup": a.warmup, "denoise_db": DEPTH, "vocoder_ms_same_batch": VOCODER_MS, "cases": {}}
    for k, v in t.items():
        xs, med = signals[k], statistics.median(v)
        frames = sum((x.size - 1) // 128 + 4 for x in xs)
        out["cases"][k] = {"signals": len(xs), "samples_each": int(xs[0].size), "stft_frames": int(frames),
                           "denoise_kernels": {"median_ms": round(med, 4), "min_ms": round(min(v), 4),
                                               "max_ms": round(max(v), 4)}}
        if k == "batch":
            out["cases"][k]["denoise_over_vocoder"] = round(med / VOCODER_MS, 4)
    x = signals["long"][0]
    t0 = time.perf_counter()
    ref = denoise_ref.denoise(x, DEPTH)
    out["numpy_contract_41s_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    y = dn.denoise(x, DEPTH)
    out["long_is_bitwise_the_contract"] = bool(np.array_equal(ref.view(np.uint32), y.view(np.uint32)))
    dn.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
