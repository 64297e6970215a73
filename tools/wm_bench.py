"""Watermark timings: nothing here is gated, these are the baseline numbers -- there is no
earlier implementation to compare with.

  embed batch   the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz), a key
                and a payload each, through one embed_batch call: the HIP-event time of the launch and the
                call's wall time (copies included), medians after a warm-up;
  embed long    one 41 s utterance (656,000 samples);
  detect batch  32 clips of 10 s through one detect_batch call: the HIP-event time of the four launches
                (whiten, fold, search, pick) and the call's wall time; the search is NP * NP * 2 adds per
                clip, given as adds per second of the whole sequence's kernel time;
  detect long   one 41 s clip;
  cpu           the same signals through the numpy restatement (tests/wm_ref.py), one timed run each: the
                embedder op for op in f32 (bitwise equality with the GPU is recorded), the detector in
                float64 with the search by FFT (equality of the decisions is recorded).
Usage: wm_bench.py [--out FILE.json] [--reps N] [--warmup N] [--no-cpu]"""
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

import rwkvtts  # noqa: E402
import wm_ref  # noqa: E402
from rwkvtts import audio  # noqa: E402

B, N = 32, 512 * 320
N_LONG = 41 * 16000
N_CLIP = 10 * 16000
KEY = 0x5EED0C0FFEE


def _speechlike(rng, n):
    """Harmonics of a wandering pitch under a slow envelope with pauses, plus a little noise."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * np.clip(np.sin(2 * np.pi * 3.1 * t) + 0.3, 0.0, None)
    x = x * (np.sin(2 * np.pi * 0.21 * t + rng.uniform(0, 6.28)) > -0.8)
    return (rng.uniform(0.02, 0.4) * x + 0.001 * rng.standard_normal(n)).astype(np.float32)


def timed(wm, call, reps, warmup):
    for _ in range(warmup):
        call()
    k, w, out = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(wm.kernel_ms())
    return out, {"kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
                 "kernel_ms_max": round(max(k), 4), "call_wall_ms_median": round(statistics.median(w), 3)}


def embed_row(wm, signals, reps, warmup, cpu):
    keys, pays = [KEY + i for i in range(len(signals))], [(0x1234 + 77 * i) & 0xFFFF for i in range(len(signals))]
    outs, row = timed(wm, lambda: wm.embed_batch(signals, keys, pays), reps, warmup)
    n = sum(x.size for x in signals)
    row["samples"] = n
    row["samples_per_s_of_kernel_time"] = round(n / (row["kernel_ms_median"] * 1e-3), 1)
    if cpu:
        t0 = time.perf_counter()
        ref = [wm_ref.embed(x, k, p) for x, k, p in zip(signals, keys, pays)]
        row["cpu"] = {"numpy_restatement_ms": round((time.perf_counter() - t0) * 1e3, 1),
                      "bitwise_equal_to_gpu": bool(all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                                                       for a, b in zip(ref, outs)))}
    return outs, row


def detect_row(wm, clips, reps, warmup, cpu):
    keys = [KEY + i for i in range(len(clips))]
    got, row = timed(wm, lambda: wm.detect_batch(clips, keys), reps, warmup)
    adds = 2.0 * wm.period * wm.period * len(clips)
    row["samples"] = sum(x.size for x in clips)
    row["search_adds"] = adds
    row["search_adds_per_s_of_kernel_time"] = round(adds / (row["kernel_ms_median"] * 1e-3), 1)
    row["detected"] = sum(1 for g in got if g["detected"])
    row["score_min"], row["score_max"] = round(min(g["score"] for g in got), 1), round(max(g["score"] for g in got), 1)
    if cpu:
        t0 = time.perf_counter()
        ref = [wm_ref.detect(x, k) for x, k in zip(clips, keys)]
        row["cpu"] = {"numpy_float64_fft_ms": round((time.perf_counter() - t0) * 1e3, 1),
                      "decisions_equal_to_gpu": bool(all((g["detected"], g["offset"], g["payload"], g["seen"]) ==
                                                         (r["detected"], r["offset"], r["payload"], r["seen"])
                                                         for g, r in zip(got, ref)))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    wm = audio.Watermarker(device=0)
    res = {"embed_batch_shape": f"{B} x {N} samples @ 16 kHz", "long_shape": f"1 x {N_LONG} samples @ 16 kHz",
           "detect_batch_shape": f"{B} x {N_CLIP} samples @ 16 kHz", "block": wm.block, "taps": wm.taps, "bits": wm.bits,
           "bit_len": wm.bit_len, "period": wm.period, "threshold": wm.threshold, "reps": a.reps, "warmup": a.warmup,
           "build_id": rwkvtts._ffi.build_id()}
    batch = [_speechlike(rng, N) for _ in range(B)]
    marked, res["embed_batch"] = embed_row(wm, batch, a.reps, a.warmup, not a.no_cpu)
    long_ = [_speechlike(rng, N_LONG)]
    marked_long, res["embed_long"] = embed_row(wm, long_, a.reps, a.warmup, not a.no_cpu)
    res["detect_batch"] = detect_row(wm, [y[:N_CLIP] for y in marked], a.reps, a.warmup, not a.no_cpu)
    res["detect_long"] = detect_row(wm, marked_long, a.reps, a.warmup, not a.no_cpu)
    wm.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
