"""Weight-format timings of the LM forward pass: the synthetic 0.4B bf16 weights with all
24 layers quantised, every layer through the separate launches. Types: none (with the persistent decode
forms switched off, so that like is compared with like), int8, nf4, mxfp8, mxfp4, mxfp6_e2m3, mxfp6_e3m2,
mxint8. Nothing here is gated.

  decode32  ms per decode step, 32 requests x S semantic tokens, graph replay: the engine's own HIP-event
            decode time over its step count (rwkvtts_get_stats);
  decode1   the same with one request;
  prefill   ms per 1280-row step: one rt.infer call of 1280 tokens (option Last, one logits row), host
            clock around the call, which ends in the logits' device-to-host copy;
  bytes     bytes of the six quantised matrices per layer as the GEMMs stream them (codes and scales;
            none: the 16-bit fragments).
The engines stay alive together and each repetition visits every type in turn, so a drift of the machine
falls on all of them. The report keeps every repetition and the median.
Usage: mx_bench.py [--out FILE.json] [--reps N] [--steps S] [--types a,b,...]"""
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
from rwkvtts import _ffi  # noqa: E402
from rwkvtts import weights as W  # noqa: E402

D = W.DIMS_04B
ROWS = 1280


def layer_bytes(qt):
    C, F = D["n_embd"], D["n_ffn"]
    elems = 4 * C * C + 2 * F * C
    return {"none": 2 * elems,
            "int8": elems + elems // 128 * 4,                # u8 codes, f16 (min, max) per 128
            "nf4": elems // 2 + elems // 64 * 2,             # nibbles, f16 absmax per 64
            "mxfp8": elems // 2048 * (2048 + 64),            # superblocks of 16 x 128: codes + 64 scale bytes
            "mxfp4": elems // 2048 * (1024 + 64),
            "mxfp6_e2m3": elems // 2048 * (1536 + 64),       # a nibble plane and a 2-bit plane
            "mxfp6_e3m2": elems // 2048 * (1536 + 64),
            "mxint8": elems // 2048 * (2048 + 64)}[qt]


def requests(n, steps):
    out = []
    for i in range(n):
        rs = np.random.RandomState(1000 + i)
        out.append(rwkvtts.TtsBatchRequest(text_tokens=rs.randint(12293, 77822, size=24).tolist(),
                                           property_tokens=[77823, 77838, 77869, 77845, 77830, 77826],
                                           args=rwkvtts.SamplerArgs(seed=i), fixed_semantic=steps))
    return out


def decode_ms(rt, reqs):
    rt.generate_batch(reqs)
    st = rt.stats()
    return st["decode_ms"] / max(st["steps"], 1)


def prefill_ms(rt, toks):
    rt.reset_slot(0)
    t0 = time.perf_counter()
    rt.infer(rwkvtts.RnnInput([rwkvtts.RnnInputBatch(list(toks), rwkvtts.RnnOption.Last)], ROWS), head_rows=8193, slots=[0])
    return (time.perf_counter() - t0) * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--types", default="none,int8,nf4,mxfp8,mxfp4,mxfp6_e2m3,mxfp6_e3m2,mxint8")
    opt = ap.parse_args()
    types = opt.types.split(",")
    blob = W.synth_blob(D, seed=20251205)
    engines = {}
    for qt in types:
        engines[qt] = rwkvtts.SharedRwkvRuntime(
            blob, max_slots=32, token_chunk_size=ROWS, use_graphs=True, quant_type=qt,
            quant_layers=D["n_layer"] if qt != "none" else 0,
            forms=(_ffi.FORM_SEPARATE_ATT | _ffi.FORM_SEPARATE_FFN) if qt == "none" else 0)
    del blob
    r32, r1 = requests(32, opt.steps), requests(1, opt.steps)
    toks = np.random.RandomState(7).randint(0, D["n_vocab"], size=ROWS).tolist()
    runs = {qt: {"decode32": [], "decode1": [], "prefill": []} for qt in types}
    for rep in range(opt.reps + 1):  # repetition 0 warms every shape up and is dropped
        for qt in types:
            rt = engines[qt]
            got = {"decode32": decode_ms(rt, r32), "decode1": decode_ms(rt, r1), "prefill": prefill_ms(rt, toks)}
            if rep:
                for k, v in got.items():
                    runs[qt][k].append(round(v, 4))
    report = {"model": "synthetic 0.4B bf16, 24 layers quantised, separate launches", "reps": opt.reps,
              "decode_steps": opt.steps, "prefill_rows": ROWS, "types": {}}
    for qt in types:
        engines[qt].close()
        report["types"][qt] = {"layer_bytes": layer_bytes(qt),
                               **{k + "_ms": {"median": round(statistics.median(v), 4), "runs": v}
                                  for k, v in runs[qt].items()}}
        t = report["types"][qt]
        print(f"{qt:6s} decode32 {t['decode32_ms']['median']:.4f} ms/step  decode1 {t['decode1_ms']['median']:.4f} ms/step  "
              f"prefill {t['prefill_ms']['median']:.3f} ms/{ROWS} rows  {t['layer_bytes'] / 2 ** 20:.2f} MiB/layer", flush=True)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
