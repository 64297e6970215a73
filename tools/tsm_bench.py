"""Time-stretch timings: nothing here is gated, these are the baseline numbers.

  batch    the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz), at
           tempo 0.8 and 1.25 through one stretch_batch call: the HIP-event time of the launch pair
           (search + overlap-add) and the call's wall time (copies included), medians after a warm-up;
  chain    one 41 s signal (656,000 samples) at tempo 0.5: the longest sequential chain -- one
           workgroup walks every frame of the signal in order;
  vocoder  (--vocoder) the wall time of one decode_audio call of the full-dims synthetic vocoder for
           the same 41 s utterance (2,050 frames), to set the chain's wall time against.
Usage: tsm_bench.py [--out FILE.json] [--reps N] [--warmup N] [--vocoder]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwkv-tts-rs_amd"))
import numpy as np  # noqa: E402

import rwkvtts  # noqa: E402
from rwkvtts import audio  # noqa: E402

B, N = 32, 512 * 320
N_LONG = 41 * 16000


def _speechlike(rng, n):
    """Harmonics of a wandering pitch under a slow envelope, plus a little noise."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t))
    return (0.2 * x + 0.01 * rng.standard_normal(n)).astype(np.float32)


def timed(ts, signals, tempos, reps, warmup):
    for _ in range(warmup):
        ts.stretch_batch(signals, tempos)
    k, w = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ts.stretch_batch(signals, tempos)
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(ts.kernel_ms())
    n_out = sum(o.size for o in out)
    frames = sum(-(-o.size // ts.hop) for o in out)
    return {"outputs": n_out, "frames": frames, "kernel_ms_median": round(statistics.median(k), 4),
            "kernel_ms_min": round(min(k), 4), "kernel_ms_max": round(max(k), 4),
            "call_wall_ms_median": round(statistics.median(w), 3),
            "us_per_frame_of_one_signal": round(statistics.median(k) * 1e3 / (frames / len(signals)), 3)}


def vocoder_row(reps, warmup):
    from rwkvtts import codec as CC
    d = CC.CODEC_DIMS_FULL
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(d), d)
    q = np.random.default_rng(3)
    T = N_LONG // 320
    g, sem = q.integers(0, 4096, d["n_global"]), q.integers(0, 8192, T)
    for _ in range(warmup):
        voc.decode_audio(g, sem)
    w = []
    for _ in range(reps):
        t0 = time.perf_counter()
        voc.decode_audio(g, sem)
        w.append((time.perf_counter() - t0) * 1e3)
    voc.close()
    return {"frames": T, "call_wall_ms_median": round(statistics.median(w), 3), "call_wall_ms_min": round(min(w), 3),
            "call_wall_ms_max": round(max(w), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocoder", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ts = audio.TimeStretcher(device=0)
    res = {"batch": f"{B} x {N} samples @ 16 kHz", "chain": f"1 x {N_LONG} samples @ 16 kHz", "window": ts.window,
           "search": ts.search, "reps": a.reps, "warmup": a.warmup, "build_id": rwkvtts._ffi.build_id(), "tempo": {}}
    batch = [_speechlike(rng, N) for _ in range(B)]
    for tempo in (0.8, 1.25):
        res["tempo"][str(tempo)] = timed(ts, batch, [tempo] * B, a.reps, a.warmup)
    res["chain_tempo_0.5"] = timed(ts, [_speechlike(rng, N_LONG)], [0.5], a.reps, a.warmup)
    ts.close()
    if a.vocoder:
        res["vocoder_one_41s_utterance"] = vocoder_row(a.reps, a.warmup)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
