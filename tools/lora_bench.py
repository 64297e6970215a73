"""Cost of per-request LoRA adapters in the LM forward pass: the synthetic 0.4B bf16 model
on ONE engine with RWKVTTS_FORM_SEPARATE_ATT | RWKVTTS_FORM_SEPARATE_FFN -- the separate launches, the
path adapter rows share, not the persistent step -- and 32 adapters of rank 16 and 32 of rank 64 resident.

  none   no row bound (the yardstick: the same launches without k_lora);
  one    every row on one adapter;
  many   row i on adapter i (32 adapters: decode32 has one row per tile, prefill 32 tiles of 40 rows).

  decode32  ms per decode step, 32 requests x S semantic tokens, graph replay: the engine's own HIP-event
            decode time over its step count (rwkvtts_get_stats);
  decode1   the same with one request (many = one there, not run);
  prefill   ms per 1280-row step: one rt.infer call of 32 slots x 40 tokens (option Last), host clock
            around the call, which ends in the logits' device-to-host copy.
Each repetition visits every configuration in turn, so a drift of the machine falls on all of them. The
report keeps every repetition and the median. Adapter values are random; timing does not depend on them.
Usage: lora_bench.py [--out FILE.json] [--reps N] [--steps S]"""
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
SLOTS, SEG = 32, 40
RANKS = (16, 64)


def adapter_blob(rank):
    rs = np.random.RandomState(rank)
    sd = {}
    for layer in range(D["n_layer"]):
        for t, name in enumerate(W.ADAPTER_TARGETS):
            N, K = W.adapter_target_shape(D, t)
            sd[f"blocks.{layer}.{name}.lora_A"] = (0.05 * rs.standard_normal((rank, K))).astype(np.float32)
            sd[f"blocks.{layer}.{name}.lora_B"] = (0.05 * rs.standard_normal((N, rank))).astype(np.float32)
    return W.pack_adapter(sd, D, alpha=float(rank))


def requests(n, steps, adapters):
    out = []
    for i in range(n):
        rs = np.random.RandomState(1000 + i)
        out.append(rwkvtts.TtsBatchRequest(text_tokens=rs.randint(12293, 77822, size=24).tolist(),
                                           property_tokens=[77823, 77838, 77869, 77845, 77830, 77826],
                                           args=rwkvtts.SamplerArgs(seed=i), fixed_semantic=steps, adapter=adapters[i]))
    return out


def decode_ms(rt, reqs):
    rt.generate_batch(reqs)
    st = rt.stats()  # (of this call: generate starts them afresh)
    return st["decode_ms"] / max(st["steps"], 1)


def prefill_ms(rt, segs, adapters):
    for s in range(SLOTS):
        rt.reset_slot(s)
        rt.set_slot_adapter(s, adapters[s])
    inp = rwkvtts.RnnInput([rwkvtts.RnnInputBatch(list(t), rwkvtts.RnnOption.Last) for t in segs], SLOTS * SEG)
    t0 = time.perf_counter()
    rt.infer(inp, head_rows=8193, slots=list(range(SLOTS)))
    ms = (time.perf_counter() - t0) * 1000
    for s in range(SLOTS):
        rt.set_slot_adapter(s, None)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    opt = ap.parse_args()
    rt = rwkvtts.SharedRwkvRuntime(W.synth_blob(D, seed=20251205), max_slots=SLOTS, token_chunk_size=SLOTS * SEG,
                                   use_graphs=True, forms=_ffi.FORM_SEPARATE_ATT | _ffi.FORM_SEPARATE_FFN)
    for k, rank in enumerate(RANKS):  # ids [32 k, 32 k + 32): one blob per rank, 32 resident copies
        blob = adapter_blob(rank)
        for i in range(SLOTS):
            rt.load_adapter(SLOTS * k + i, blob)
    configs = {"none": [None] * SLOTS}
    for k, rank in enumerate(RANKS):
        configs[f"one_r{rank}"] = [SLOTS * k] * SLOTS
        configs[f"many_r{rank}"] = [SLOTS * k + i for i in range(SLOTS)]
    rs = np.random.RandomState(7)
    segs = [rs.randint(0, D["n_vocab"], size=SEG).tolist() for _ in range(SLOTS)]
    runs = {c: {"decode32": [], "decode1": [], "prefill": []} for c in configs}
    for rep in range(opt.reps + 1):  # repetition 0 warms every shape up and is dropped
        for c, ads in configs.items():
            got = {"decode32": decode_ms(rt, requests(SLOTS, opt.steps, ads)), "prefill": prefill_ms(rt, segs, ads)}
            if not c.startswith("many"):
                got["decode1"] = decode_ms(rt, requests(1, opt.steps, ads))
            if rep:
                for k, v in got.items():
                    runs[c][k].append(round(v, 4))
    rt.close()
    report = {"model": "synthetic 0.4B bf16, separate launches, 64 adapters resident", "reps": opt.reps,
              "decode_steps": opt.steps, "prefill_rows": SLOTS * SEG, "configs": {}}
    for c in configs:
        report["configs"][c] = {k + "_ms": {"median": round(statistics.median(v), 4), "runs": v} for k, v in runs[c].items() if v}
        print(c, " ".join(f"{k} {v['median']:.4f}" for k, v in report["configs"][c].items()), flush=True)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
