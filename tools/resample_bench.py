"""Resampler timings: nothing here is gated, these are the baseline numbers.

  kernel   the bench-shaped batch, 32 utterances x 512 frames (32 x 163,840 samples at 16 kHz), to 8,
           24, 44.1 and 48 kHz through one resample_batch call: the kernel's own HIP-event time and the
           call's wall time (host -> device copy, kernel, device -> host copy), medians after a warm-up;
  numpy    one utterance of the same batch through audio.resample_audio_high_quality's numpy path on
           the host (one run per rate), and that time x 32 as the batch's extrapolation;
  ttfa     (--ttfa) first-chunk latency of one streamed request as tools/ttfa_bench.py measures it
           (0.4B synthetic model, full-dims synthetic vocoder, S tokens, 16-frame chunks), with and
           without sample_rate=48000, alternating in one process.
Usage: resample_bench.py [--out FILE.json] [--reps N] [--warmup N] [--ttfa] [--S TOKENS] [--no-numpy]"""
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

RATES = (8000, 24000, 44100, 48000)
B, N = 32, 512 * 320


def kernel_rows(reps, warmup):
    rs = np.random.default_rng(0)
    batch = [(rs.standard_normal(N) * 0.3).astype(np.float32) for _ in range(B)]
    rows = {}
    for rate in RATES:
        r = audio.Resampler(16000, rate, device=0, align="zero")
        for _ in range(warmup):
            r.resample_batch(batch)
        k, w = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = r.resample_batch(batch)
            w.append((time.perf_counter() - t0) * 1e3)
            k.append(r.kernel_ms())
        n_out = sum(o.size for o in out)
        rows[str(rate)] = {"outputs": n_out, "kernel_ms_median": round(statistics.median(k), 4),
                           "kernel_ms_min": round(min(k), 4), "kernel_ms_max": round(max(k), 4),
                           "call_wall_ms_median": round(statistics.median(w), 3),
                           "gmac_per_s": round(n_out * 2 * r.sinc_len / statistics.median(k) / 1e6, 1)}
        r.close()
    return rows, batch[0]


def numpy_rows(x):
    rows = {}
    for rate in RATES:
        t0 = time.perf_counter()
        audio.resample_audio_high_quality(x, 16000, rate)
        dt = time.perf_counter() - t0
        rows[str(rate)] = {"one_utterance_s": round(dt, 3), "batch_of_32_extrapolated_s": round(dt * B, 2)}
    return rows


def ttfa_rows(S, reps):
    from rwkvtts import codec as CC
    from rwkvtts import weights as W
    from rwkvtts.pipeline import LightweightTtsPipeline
    props = [77823, 77838, 77869, 77845, 77830, 77826]
    blob = W.synth_blob(W.DIMS_04B, seed=20251205)
    mgr = rwkvtts.DynamicBatchManager(blob, config=rwkvtts.DynamicBatchConfig(max_batch_size=32, collect_timeout_ms=2),
                                      devices=[0], max_slots=32, token_chunk_size=512)
    del blob
    d = CC.CODEC_DIMS_FULL
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(d), d)
    pipe = LightweightTtsPipeline(mgr, voc)
    q = np.random.RandomState(1007)
    req = rwkvtts.TtsBatchRequest(text_tokens=q.randint(12293, 77822, size=24).tolist(), property_tokens=props,
                                  args=rwkvtts.SamplerArgs(seed=7), fixed_semantic=S)

    def streamed(rate):
        t0 = time.perf_counter()
        first = last = None
        n = 0
        for c in pipe.stream_request(req, 16, sample_rate=rate):
            last = time.perf_counter() - t0
            first = last if first is None else first
            n += c.size
        return first * 1e3, last * 1e3, n

    for rate in (None, 48000):
        streamed(rate)  # warm-up: graphs captured, buffers sized, the resampler created
    rows = {"16000": [], "48000": []}
    for _ in range(reps):
        for rate in (None, 48000):
            rows[str(rate or 16000)].append(streamed(rate))
    out = {"S": S, "chunk_frames": 16, "reps": reps}
    for k, v in rows.items():
        out[k] = {"first_chunk_ms_median": round(statistics.median(r[0] for r in v), 3),
                  "first_chunk_ms_all": [round(r[0], 3) for r in v],
                  "last_chunk_ms_median": round(statistics.median(r[1] for r in v), 3), "samples": v[0][2]}
    mgr.close()
    voc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ttfa", action="store_true")
    ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    res = {"batch": f"{B} x {N} samples @ 16 kHz", "reps": a.reps, "warmup": a.warmup,
           "build_id": rwkvtts._ffi.build_id()}
    res["kernel"], x = kernel_rows(a.reps, a.warmup)
    if not a.no_numpy:
        res["numpy"] = numpy_rows(x)
    if a.ttfa:
        res["ttfa"] = ttfa_rows(a.S, 5)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
