"""Formant-shift timings, modelled on pitch_bench.py: nothing here is gated. One process
times, in alternating repetitions, the pitch-only calls (+4 and 0 semitones: k_pitch_synth) and the formant
calls (pitch 0, formant +4 and -4: k_formant_synth) on the same signals, so the two paths share the
machine's state; run it once more with RWKVTTS_LIB pointing at the parent commit's library and
--pitch-only to put that build's pitch path beside this one's.

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz), one
           shift_batch call: the HIP-event time of the launch triple (period + marks + synthesis) and of
           the marks kernel, medians after a warm-up. minus_pitch0_ms is a formant triple minus the
           pitch triple at 0 semitones: the same periods, marks and grains, so the difference of the
           two medians is the difference of the two synthesis kernels;
  long     one 41 s utterance (656,000 samples);
  share    the triple's kernel time against the vocoder's 51.8 ms for the same batch, and
           the LDS words the formant synthesis reads per output (32 per covering grain).
Usage: formant_bench.py [--out FILE.json] [--reps N] [--warmup N] [--pitch-only]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwkv-tts-rs_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import rwkvtts  # noqa: E402
from pitch_bench import B, N, N_LONG, VOCODER_MS, _speechlike  # noqa: E402
from rwkvtts import audio  # noqa: E402

CASES = {"pitch+4": (4.0, None), "pitch0": (0.0, None), "formant+4": (0.0, 4.0), "formant-4": (0.0, -4.0)}


def timed(ps, signals, cases, reps, warmup):
    """Alternating repetitions: every round runs each case once, in order."""
    k = {c: [] for c in cases}
    m = {c: [] for c in cases}
    for r in range(warmup + reps):
        for c in cases:
            pitch, formant = CASES[c]
            kw = {} if formant is None else {"formant": [formant] * len(signals)}
            ps.shift_batch(signals, [pitch] * len(signals), **kw)
            if r >= warmup:
                k[c].append(ps.kernel_ms())
                m[c].append(ps.walk_ms())
    return {c: {"kernel_ms_median": round(statistics.median(k[c]), 4), "kernel_ms_min": round(min(k[c]), 4),
                "kernel_ms_max": round(max(k[c]), 4), "walk_ms_median": round(statistics.median(m[c]), 4),
                "kernel_ms_over_vocoder_ms": round(statistics.median(k[c]) / VOCODER_MS, 4)} for c in cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pitch-only", action="store_true")
    a = ap.parse_args()
    cases = ["pitch+4", "pitch0"] if a.pitch_only else list(CASES)
    rng = np.random.default_rng(0)
    ps = audio.PitchShifter(device=0)
    res = {"batch_shape": f"{B} x {N} samples @ 16 kHz", "long_shape": f"1 x {N_LONG} samples @ 16 kHz", "cases": cases,
           "reps": a.reps, "warmup": a.warmup, "vocoder_ms_same_batch": VOCODER_MS, "build_id": rwkvtts._ffi.build_id(),
           "library": "alternative build (RWKVTTS_LIB)" if os.environ.get("RWKVTTS_LIB") else "in-tree"}
    res["batch"] = timed(ps, [_speechlike(rng, N) for _ in range(B)], cases, a.reps, a.warmup)
    res["long"] = timed(ps, [_speechlike(rng, N_LONG)], cases, a.reps, a.warmup)
    ps.close()
    if not a.pitch_only:
        for part in ("batch", "long"):
            for c in ("formant+4", "formant-4"):
                res[part][c]["minus_pitch0_ms"] = round(res[part][c]["kernel_ms_median"]
                                                        - res[part]["pitch0"]["kernel_ms_median"], 4)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
