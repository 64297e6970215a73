"""High-band timings, modelled on formant_bench.py: nothing here is gated. One process
times, in alternating repetitions, on speech-like signals with a noise share (so that blocks get a
high band and the synthesis kernel does all of its work):

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz): one
           extend_batch call to 32 kHz (the HIP-event time of the launch pair, gain + synth), then one
           resample_batch call 32 kHz -> 48 kHz on its output (the resampler's kernel), medians after a
           warm-up, with min and max; beside the vocoder's 51.8 ms for the same batch;
  long     one 41 s utterance (656,000 samples), the same two calls;
  quiet    a batch of the same shape of low sines: every gain is 0, so every piece skips b and SH;
  numpy    the contract's restatement (tests/highband_ref.py) on the 41 s utterance, once, wall time;
  mark     one detector case: the speech-like signal marked (audio.Watermarker), taken to 48 kHz with and
           without the high band, brought back to 16 kHz by a 48 kHz -> 16 kHz resampler and detected:
           both scores, neither gated.
Usage: highband_bench.py [--out FILE.json] [--reps N] [--warmup N]"""
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

import highband_ref  # noqa: E402
from pitch_bench import B, N, N_LONG, VOCODER_MS, _speechlike  # noqa: E402
from rwkvtts import audio  # noqa: E402


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    hb = audio.HighBand(device=0)
    rs = audio.Resampler(32000, 48000, device=0, align="zero")
    cases = {
        "batch": [(_speechlike(rng, N) + 0.05 * rng.standard_normal(N)).astype(np.float32) for _ in range(B)],
        "long": [(_speechlike(rng, N_LONG) + 0.05 * rng.standard_normal(N_LONG)).astype(np.float32)],
        "quiet": [(0.3 * np.sin(2 * np.pi * (150.0 + 5.0 * i) * np.arange(N) / 16000.0)).astype(np.float32) for i in range(B)],
    }
    t = {c: {"highband": [], "resample_32k_48k": []} for c in cases}
    live = {}
    for r in range(a.warmup + a.reps):
        for c, xs in cases.items():  # alternating: every round runs each case once, in order
            wide = hb.extend_batch(xs, [0.0] * len(xs))
            k_hb = hb.kernel_ms()
            rs.resample_batch(wide)
            if r >= a.warmup:
                t[c]["highband"].append(k_hb)
                t[c]["resample_32k_48k"].append(rs.kernel_ms())
            live[c] = float(np.mean([np.any(w[0::2] != x) for w, x in zip(wide, xs)]))
    out = {"reps": a.reps, "warmup": a.warmup, "vocoder_ms_same_batch": VOCODER_MS, "cases": {}}
    for c in cases:
        out["cases"][c] = {"signals": len(cases[c]), "samples_each": int(cases[c][0].size),
                           "share_of_signals_with_a_high_band": live[c],
                           "highband_kernel": stats(t[c]["highband"]), "resample_kernel": stats(t[c]["resample_32k_48k"])}
    out["cases"]["batch"]["highband_over_vocoder"] = round(out["cases"]["batch"]["highband_kernel"]["median_ms"] / VOCODER_MS, 5)
    t0 = time.perf_counter()
    ref = highband_ref.highband(cases["long"][0], 0.0, tab=hb.table)
    out["numpy_contract_41s_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["long_is_bitwise_the_contract"] = bool(np.array_equal(ref.view(np.uint32), hb.extend(cases["long"][0], 0.0).view(np.uint32)))
    # the detector case
    key, payload = 0x1234ABCD5678EF01, 0xBEEF
    mk = audio.Watermarker(device=0)
    up, down = audio.Resampler(16000, 48000, device=0, align="zero"), audio.Resampler(48000, 16000, device=0, align="zero")
    marked = mk.embed(cases["long"][0][:10 * 16000], key, payload)
    res = {}
    for name, y48 in (("without_highband", up.resample(marked)), ("with_highband", rs.resample(hb.extend(marked, 0.0)))):
        d = mk.detect(down.resample(y48), key)
        res[name] = {k: (float(d[k]) if k in ("score", "threshold", "min_z") else int(d[k])) for k in
                     ("score", "threshold", "detected", "payload", "min_z")}
    out["watermark_detector_after_48k_round_trip"] = res
    for s in (hb, rs, mk, up, down):
        s.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
