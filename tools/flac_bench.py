"""FLAC encoder sizes and timings: nothing here is gated, these are the first numbers --
there is no earlier implementation to compare with.

  batch    the bench-shaped batch, 32 signals x 163,840 samples at 16 kHz, and the same signals resampled
           to 48 kHz on the GPU (audio.Resampler), through one encode_batch call each: the HIP-event time
           of the launch pair (k_flac_frame + k_flac_pack) and the call's wall time (copies and the MD5
           included), medians after a warm-up;
  signals  `vowels`: synthetic vowels (a pulse train plus breath noise through parallel formant
           resonators, a pitch, a level and a seed per signal); `vocoder`: the tiny synthetic vocoder's
           output for random tokens (noise-like: no checkpoint is in the repository);
  bytes    FLAC bytes against the PCM's 2 bytes a sample, with LPC and with FIXED only;
  cpu      the first --cpu-signals signals through the numpy restatement (tests/flac_ref.py), one timed
           run, and whether the GPU's bytes equal it;
  vocoder  the README's vocoder time for the same batch, 51.8 ms, beside the kernel time.
Usage: flac_bench.py [--out FILE.json] [--reps N] [--warmup N] [--cpu-signals N]"""
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

import flac_ref  # noqa: E402
import rwkvtts  # noqa: E402
from rwkvtts import audio  # noqa: E402
from rwkvtts import codec as CC  # noqa: E402

B, N = 32, 512 * 320
VOCODER_MS = 51.8  # README: the vocoder's time for this batch


def _vowel(rng, n, rate=16000):
    """flac_ref.vowel's signal with the resonators applied in the frequency domain (circular)."""
    f0 = rng.uniform(90.0, 220.0)
    e = np.zeros(n)
    e[(np.arange(int(n * f0 / rate)) * (rate / f0)).astype(int)] = 1.0
    e += 0.05 * rng.standard_normal(n)
    z = np.exp(-2j * np.pi * np.fft.rfftfreq(n))
    H = 0.0
    for f, bw in ((700.0, 90.0), (1200.0, 110.0), (2600.0, 160.0), (5200.0, 400.0)):
        r = np.exp(-np.pi * bw / rate)
        H = H + 1.0 / (1.0 - 2.0 * r * np.cos(2.0 * np.pi * f / rate) * z + r * r * z * z)
    y = np.fft.irfft(np.fft.rfft(e) * H, n)
    return (y * (rng.uniform(0.05, 0.6) / np.max(np.abs(y)))).astype(np.float32)


def timed(enc, signals, rate, lpc, reps, warmup):
    rates = [rate] * len(signals)
    for _ in range(warmup):
        enc.encode_batch(signals, rates, lpc=lpc)
    k, w = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = enc.encode_batch(signals, rates, lpc=lpc)
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(enc.kernel_ms())
    n = sum(x.size for x in signals)
    nbytes = sum(len(f) for f in out)
    km = statistics.median(k)
    return out, {"samples": n, "pcm_bytes": 2 * n, "flac_bytes": nbytes, "ratio": round(nbytes / (2.0 * n), 4),
                 "kernel_ms_median": round(km, 4), "kernel_ms_min": round(min(k), 4), "kernel_ms_max": round(max(k), 4),
                 "call_wall_ms_median": round(statistics.median(w), 3),
                 "samples_per_s_over_kernel_time": round(n / (km * 1e-3), 1),
                 "share_of_vocoder_ms": round(km / VOCODER_MS, 4)}


def rows(enc, signals, rate, a):
    out, row = timed(enc, signals, rate, True, a.reps, a.warmup)
    _, fixed = timed(enc, signals, rate, False, max(a.reps // 2, 1), 1)
    row["fixed_only"] = {k: fixed[k] for k in ("flac_bytes", "ratio", "kernel_ms_median")}
    if a.cpu_signals > 0:
        t0 = time.perf_counter()
        ref = [flac_ref.encode(x, rate) for x in signals[:a.cpu_signals]]
        row["cpu"] = {"signals": len(ref), "numpy_restatement_ms": round((time.perf_counter() - t0) * 1e3, 1),
                      "bitwise_equal_to_gpu": bool(all(r == g for r, g in zip(ref, out)))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-signals", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    enc = audio.FlacEncoder(device=0)
    up = audio.Resampler(16000, 48000, device=0)
    res = {"batch_shape": f"{B} x {N} samples @ 16 kHz, and resampled to 48 kHz", "blocks": {"16000": 1024, "48000": 2048},
           "reps": a.reps, "warmup": a.warmup, "vocoder_ms_readme": VOCODER_MS, "build_id": rwkvtts._ffi.build_id()}
    vowels = [_vowel(rng, N) for _ in range(B)]
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    pcm = voc.decode_audio_batch([(rng.integers(0, 4096, cd["n_global"]), rng.integers(0, cd["codebook_size"], N // 320))
                                  for _ in range(B)])
    voc.close()
    for name, sigs in (("vowels", vowels), ("vocoder", pcm)):
        res[name] = {"16000": rows(enc, sigs, 16000, a), "48000": rows(enc, up.resample_batch(sigs), 48000, a)}
    enc.close()
    up.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
