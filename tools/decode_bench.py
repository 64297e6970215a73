"""Decode-loop microbenchmark: 32 requests (0.4B synthetic bf16), fixed S semantic tokens, graph
replay. Prints decode ms/step from the engine's own HIP events and a token checksum (a kernel
change that keeps the arithmetic must keep the checksum). Usage: decode_bench.py [S] [reps]
[--temperature T] [--top-p P] [--top-k K] [--sampling-slots N]: the semantic phase's sampling
parameters (runtime.PhaseSampling; an option left out keeps the phase's own value) for the first N
requests (default: all of them); without any of the three, no request carries parameters.
[--repetition R] [--frequency F] [--presence P] [--window W] [--penalty-slots N]: the penalties
(runtime.Penalties) of the first N requests (default: all of them); without any of the first three, no
request carries penalties. The report adds the most often repeated token's count over all requests.
[--mirostat-tau T] [--mirostat-rate R] [--mirostat-slots N]: Mirostat (runtime.Mirostat; either option
selects it, the other keeps its default 3.0 / 0.1) in the semantic phase of the first N requests
(default: all of them); it excludes the three sampling options.
Env: DB_B requests (default 32), DB_F16=1 fp16 weights, DB_ZS=1 zero-shot prompts (32 reference
global tokens + 128 reference semantic tokens per request), DB_QUANT=int8|nf4 (every layer quantised,
the server's --quant-layers 24 --quant-type ...), DB_FORMS=n (rwkvtts_engine_desc.forms: RWKVTTS_FORM_* bits)."""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwkv-tts-rs_amd"))
import rwkvtts  # noqa: E402
from rwkvtts import weights as W  # noqa: E402

import argparse  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("S", nargs="?", type=int, default=64)
ap.add_argument("reps", nargs="?", type=int, default=2)
ap.add_argument("--temperature", type=float, default=None)
ap.add_argument("--top-p", type=float, default=None)
ap.add_argument("--top-k", type=int, default=None)
ap.add_argument("--sampling-slots", type=int, default=None)
ap.add_argument("--repetition", type=float, default=None)
ap.add_argument("--frequency", type=float, default=None)
ap.add_argument("--presence", type=float, default=None)
ap.add_argument("--window", type=int, default=0)
ap.add_argument("--penalty-slots", type=int, default=None)
ap.add_argument("--mirostat-tau", type=float, default=None)
ap.add_argument("--mirostat-rate", type=float, default=None)
ap.add_argument("--mirostat-slots", type=int, default=None)
opt = ap.parse_args()
S, reps = opt.S, opt.reps
sampling = None
if opt.temperature is not None or opt.top_p is not None or opt.top_k is not None:
    sampling = rwkvtts.PhaseSampling(**{k: v for k, v in (("temperature", opt.temperature), ("top_p", opt.top_p),
                                                           ("top_k", opt.top_k)) if v is not None}).check("semantic")
penalties = None
if opt.repetition is not None or opt.frequency is not None or opt.presence is not None:
    penalties = rwkvtts.Penalties(**{k: v for k, v in (("repetition", opt.repetition), ("frequency", opt.frequency),
                                                       ("presence", opt.presence)) if v is not None},
                                  window=opt.window).check()
mirostat = None
if opt.mirostat_tau is not None or opt.mirostat_rate is not None:
    if sampling is not None:
        ap.error("--mirostat-* replaces the semantic phase's top-k, top-p and temperature")
    mirostat = rwkvtts.Mirostat(**{k: v for k, v in (("tau", opt.mirostat_tau), ("rate", opt.mirostat_rate))
                                   if v is not None}).check()
f16 = os.environ.get("DB_F16", "0") == "1"
B = int(os.environ.get("DB_B", "32"))
zs = os.environ.get("DB_ZS", "0") == "1"
blob = W.synth_blob(W.DIMS_04B, seed=20251205, **({"dtype": rwkvtts._ffi.DTYPE_F16} if f16 else {}))
qt = os.environ.get("DB_QUANT", "none")
rt = rwkvtts.SharedRwkvRuntime(blob, max_slots=max(B, 1), token_chunk_size=512, use_graphs=True,
                               quant_layers=W.DIMS_04B["n_layer"] if qt != "none" else 0, quant_type=qt,
                               forms=int(os.environ.get("DB_FORMS", "0")))
del blob
import numpy as np  # noqa: E402
reqs = []
for i in range(B):
    rs = np.random.RandomState(1000 + i)
    ref = {}
    if zs:
        ref = dict(ref_global_tokens=rs.randint(0, 4096, size=32).tolist(),
                   ref_semantic_tokens=rs.randint(0, 8192, size=128).tolist())
    reqs.append(rwkvtts.TtsBatchRequest(text_tokens=rs.randint(12293, 77822, size=24).tolist(),
                                        property_tokens=[] if zs else [77823, 77838, 77869, 77845, 77830, 77826],
                                        args=rwkvtts.SamplerArgs(seed=i), fixed_semantic=S, **ref))
    if sampling is not None and i < (B if opt.sampling_slots is None else opt.sampling_slots):
        reqs[-1].args.semantic_sampling = sampling
    if penalties is not None and i < (B if opt.penalty_slots is None else opt.penalty_slots):
        reqs[-1].args.penalties = penalties
    if mirostat is not None and i < (B if opt.mirostat_slots is None else opt.mirostat_slots):
        reqs[-1].args.mirostat = mirostat
for r in range(reps):
    t0 = time.perf_counter()
    out = rt.generate_batch(reqs)
    wall = time.perf_counter() - t0
    st = rt.stats()
    h = hashlib.sha1(repr(out).encode()).hexdigest()[:12]
    us = st['decode_ms'] / max(st['steps'], 1) * 1000
    top = max((max(np.bincount(np.asarray(s, dtype=np.int64), minlength=1)) for _, s in out if len(s)), default=0)
    print(f"rep {r}: B={B} f16={int(f16)} zs={int(zs)} quant={qt} sampling={sampling} penalties={penalties} mirostat={mirostat} "
          f"max_repeat={top} decode {us:.1f} us/step over {st['steps']} steps "
          f"({B * 320 / us * 1e6:.0f} samples/s decode-only), "
          f"prefill {st['prefill_ms']:.2f} ms, wall {wall * 1000:.1f} ms, tokens {h}", flush=True)
rt.close()
