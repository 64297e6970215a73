"""Long-form synthesis timings: nothing here is gated, these are the baseline numbers.

  join     32 jobs x 8 segments x 80,000 samples (5 s each at 16 kHz, silent head and tail) through one
           join_batch call with the default keep / fade: the HIP-event time of the kernels (bounds,
           layout, write) and the call's wall time (copies included), medians after a warm-up;
  long     the wall time of generate_long_speech for a text of 32 segments on the synthetic 0.4B
           weights and the full-dims synthetic vocoder (32 slots, one engine), against the same 32
           segment texts run one after another through generate_speech -- the only way the library
           offered before. Synthetic weights end a request where they happen to, so max_tokens bounds
           every segment; the semantic tokens each way produced are reported beside the times.
Usage: long_bench.py [--out FILE.json] [--reps N] [--warmup N] [--max-tokens N] [--skip-long]"""
import argparse
import dataclasses
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

JOBS, SEGS, N = 32, 8, 80000
N_SEGMENTS = 32
WORDS = ("river", "morning", "window", "between", "quiet", "station", "yellow", "paper", "remember", "silver",
         "garden", "letter", "evening", "distant", "travel", "kitchen", "number", "simple", "winter", "market")


def _segment_pcm(rng, n):
    """0.4 s of near-silence, speech-level noise, 0.6 s of near-silence."""
    x = (rng.standard_normal(n) * 0.001).astype(np.float32)
    x[6400:n - 9600] = (rng.standard_normal(n - 16000) * 0.2).astype(np.float32)
    return x


def join_row(reps, warmup):
    rng = np.random.default_rng(0)
    j = audio.Joiner(device=0)
    jobs = [([_segment_pcm(rng, N) for _ in range(SEGS)], [4800] * (SEGS - 1) + [0]) for _ in range(JOBS)]
    for _ in range(warmup):
        j.join_batch(jobs)
    k, w = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = j.join_batch(jobs)
        w.append((time.perf_counter() - t0) * 1e3)
        k.append(j.kernel_ms())
    j.close()
    n_in = JOBS * SEGS * N
    return {"shape": f"{JOBS} jobs x {SEGS} segments x {N} samples", "keep": 800, "fade": 80,
            "samples_in": n_in, "samples_out": int(sum(y.size for y, _ in out)),
            "kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
            "kernel_ms_max": round(max(k), 4), "call_wall_ms_median": round(statistics.median(w), 3),
            "kernel_gb_per_s": round(2 * 4 * n_in / (statistics.median(k) * 1e-3) / 1e9, 1)}


def long_text(tok, segment_tokens):
    """32 sentences, each within the budget and too long to share a segment with its neighbour."""
    from rwkvtts.segment import split_text
    rng = np.random.default_rng(1)
    sentences = []
    for _ in range(N_SEGMENTS):
        words = []
        while len(tok.encode(" ".join(words + ["x"]) + ".")) < segment_tokens * 3 // 4:
            words.append(WORDS[int(rng.integers(len(WORDS)))])
        sentences.append(" ".join(words).capitalize() + ".")
    text = " ".join(sentences)
    segs = split_text(text, tok.encode, segment_tokens)
    assert len(segs) == N_SEGMENTS, len(segs)
    return text, segs


def long_row(reps, warmup, max_tokens):
    from rwkvtts import codec as CC
    from rwkvtts import weights as W
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from rwkvtts.tokenizer import Tokenizer
    tok = Tokenizer(os.path.join(ROOT, "rwkv-tts-rs_amd", "assets", "tokenizer.json"))
    m = rwkvtts.DynamicBatchManager(W.synth_blob(W.DIMS_04B), devices=[0], max_slots=32, token_chunk_size=512,
                                    tokenizer=tok)
    cd = CC.CODEC_DIMS_FULL
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd), cd)
    pipe = LightweightTtsPipeline(m, voc)
    text, segs = long_text(tok, 64)
    args = LightweightTtsPipelineArgs(text=text, seed=7, max_tokens=max_tokens)

    def one_call():
        t0 = time.perf_counter()
        out = pipe.generate_long_speech(args)
        return (time.perf_counter() - t0) * 1e3, sum(s["n_semantic"] for s in out.segments), out.size

    def one_by_one():
        t0 = time.perf_counter()
        n = 0
        for i, s in enumerate(segs):
            n += pipe.generate_speech(dataclasses.replace(args, text=s.text.strip(), seed=7 + i)).size
        return (time.perf_counter() - t0) * 1e3, n

    for _ in range(warmup):
        one_call()
        one_by_one()
    a = [one_call() for _ in range(reps)]
    b = [one_by_one() for _ in range(reps)]
    m.close()
    voc.close()
    la, lb = statistics.median(x[0] for x in a), statistics.median(x[0] for x in b)
    return {"segments": N_SEGMENTS, "text_tokens": sum(len(s.tokens) for s in segs), "max_tokens": max_tokens,
            "weights": "synthetic 0.4B, bf16", "slots": 32,
            "long_wall_ms_median": round(la, 1), "long_semantic_tokens": a[-1][1], "long_samples": a[-1][2],
            "sequential_wall_ms_median": round(lb, 1), "sequential_samples": b[-1][1],
            "speedup": round(lb / la, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-tokens", type=int, default=256)
    ap.add_argument("--skip-long", action="store_true")
    a = ap.parse_args()
    res = {"reps": a.reps, "warmup": a.warmup, "build_id": rwkvtts._ffi.build_id(), "join": join_row(a.reps, a.warmup)}
    if not a.skip_long:
        res["long"] = long_row(max(a.reps // 2, 1), 1, a.max_tokens)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
