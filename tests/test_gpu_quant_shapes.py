"""Int8 / NF4 layers (k_quant_pack, the QW forms of gemm2_body) at the row counts, steps and scales
tests/test_gpu_quant.py does not run, against a float64 model of the quantised network.

forward_check.check_case unchanged, all three assertions (float64; bitwise against the segment alone;
bitwise against one token per call), the reference being Reference(quant_ref.quantised_model(...)):
rwkv7_f64 with the numpy restatement's dequantised matrices. use_graphs=False, max_slots=4, n_vocab 8209,
head_rows 200. Gates are test_gpu_forward_dims.py's: logits 2e-3 * max(1, sigma / 1.6), state 1e-3.

  set    quantised layers  what it reaches
  tiny   2 of 2            every split 1; all of {int8, nf4} x {bf16, f16}
  c384   2 of 2            key split 3: the pre-summed slab up to 64 rows, relu^2 planes beyond (bf16; f16
                           always sums); int8-bf16, nf4-f16
  mid    1 of 2            C = 1024, 256-deep slices, split-K; quantised separate launches feed the
                           unquantised layer; nf4-bf16, int8-f16 (the complement of test_gpu_quant.py)

Rows 1 (a decode row), 16 (a full MT 1 tile), 17 / 32 (two tiles: the range the unquantised path gives
the 16 x 128 value role and QW does not), 33 (a second row group, one group per workgroup), 65 (past
the 64-row planes switch); mid keeps 1 / 17 / 33 / 65. One ragged step (5 / 16 / 23 / 1 rows in one
call, the third OPT_LAST) and one 40-token prompt in chunks of 16.

Guard (CPU, when a case is built): the float64 quantised model's logits differ from the float64 16-bit
model's by at least 50 gates on the probe tokens, so a kernel that ignored the codes or read another
block's scale cannot pass. Plain synthetic weights (normal, sigma 0.02) miss it: Int8 moves their logits by
under one gate. Every blob here is therefore redrawn with a larger spread (_spread: one outlier of 16
times per 32 weights, the matrices times 4), chosen on the CPU from the guard and the state's magnitude
(STATE_TOP below: the largest float64 state a case may have, asserted with the guard).

f16 shift cases (tiny, both types, both layers quantised): Engine::init computes one q_shift per launch
from the launch's largest scale.
  small   the six quantised matrices of layer 0 times 2^-14, so shift_of reaches its clamp of 24. The
          product is NOT exact in f16 (a weight of 0.02 has bits down to 2^-16; 2^-14 of it needs 2^-30,
          f16 ends at 2^-24): the blob holds the products rounded to f16 (nearest even), about +-100
          steps of 2^-24, and the reference is built from that blob. Asserted instead: every edited
          matrix is non-zero and its largest magnitude is at most 2^-11, for which the unclamped shift
          is 25 or more.
  uneven  wv and ffn_value of layer 0 times 2^-8 (rounded to f16 likewise): the rkv launch's shift is
          set by wr / wk while wv's dequantised weights sit 2^8 lower in the f16 hi / lo split.
Each on 1 and 17 rows, same gates, same guard: layer 0 scaled down moves the logits less, so these blobs
give layer 1 a wider spread (one outlier of 64 times per 128 weights; 99 / 169 gates for Int8 small /
uneven, over 700 for NF4). For `small`, a guard of layer 0's matrices against the same model with them
zeroed cannot be reached at any spread: behind GroupNorm's eps and three factors of 2^-14 they move the
float64 logits by about 1e-6, under a thousandth of a gate. What they do leave is layer 0's WKV state, at
2^-28 of its usual size; test_f16_shift compares that relative to its largest entry (bound 1e-3), which
holds the rkv launch's shift for both variants. Wo's and the FFN launches' clamped shift in `small` is held
only by the bitwise assertions and the absence of Inf / NaN.

Measured on an MI355X (FWD-ERR lines of check_case: worst logit / state error against float64):
  quant tiny bf16 int8 single[1] logit 1.17e-05 state 6.45e-05
  quant tiny bf16 int8 single[16] logit 2.42e-05 state 0.000254
  quant tiny bf16 int8 single[17] logit 2.53e-05 state 0.000306
  quant tiny bf16 int8 single[32] logit 2.72e-05 state 0.000246
  quant tiny bf16 int8 single[33] logit 2.27e-05 state 0.000198
  quant tiny bf16 int8 single[65] logit 3.63e-05 state 0.000521
  quant tiny f16 int8 single[1] logit 7.22e-07 state 6.15e-06
  quant tiny f16 int8 single[16] logit 1.12e-06 state 8.64e-06
  quant tiny f16 int8 single[17] logit 1.36e-06 state 1.35e-05
  quant tiny f16 int8 single[32] logit 1.25e-06 state 1.1e-05
  quant tiny f16 int8 single[33] logit 1.16e-06 state 1.79e-05
  quant tiny f16 int8 single[65] logit 1.28e-06 state 1.55e-05
  quant tiny bf16 nf4 single[1] logit 1.33e-05 state 6.9e-05
  quant tiny bf16 nf4 single[16] logit 2.05e-05 state 0.000324
  quant tiny bf16 nf4 single[17] logit 1.94e-05 state 0.000492
  quant tiny bf16 nf4 single[32] logit 2.35e-05 state 0.000224
  quant tiny bf16 nf4 single[33] logit 1.97e-05 state 0.000331
  quant tiny bf16 nf4 single[65] logit 3.24e-05 state 0.000316
  quant tiny f16 nf4 single[1] logit 8.15e-07 state 8.24e-06
  quant tiny f16 nf4 single[16] logit 8.6e-07 state 9.52e-06
  quant tiny f16 nf4 single[17] logit 9.97e-07 state 1.86e-05
  quant tiny f16 nf4 single[32] logit 1.23e-06 state 1.01e-05
  quant tiny f16 nf4 single[33] logit 8.17e-07 state 1.68e-05
  quant tiny f16 nf4 single[65] logit 1.23e-06 state 1.37e-05
  quant c384 bf16 int8 single[1] logit 1.9e-05 state 2.47e-05
  quant c384 bf16 int8 single[16] logit 3.43e-05 state 0.000111
  quant c384 bf16 int8 single[17] logit 3.15e-05 state 0.000115
  quant c384 bf16 int8 single[32] logit 0.000237 state 0.000148
  quant c384 bf16 int8 single[33] logit 3.83e-05 state 0.000194
  quant c384 bf16 int8 single[65] logit 3.95e-05 state 0.000153
  quant c384 f16 nf4 single[1] logit 1.44e-06 state 2.62e-06
  quant c384 f16 nf4 single[16] logit 1.51e-06 state 5.61e-06
  quant c384 f16 nf4 single[17] logit 1.72e-06 state 5.63e-06
  quant c384 f16 nf4 single[32] logit 1.29e-05 state 1.2e-05
  quant c384 f16 nf4 single[33] logit 1.58e-06 state 6.42e-06
  quant c384 f16 nf4 single[65] logit 1.63e-06 state 6.11e-06
  quant mid bf16 nf4 single[1] logit 4.7e-05 state 4.94e-05
  quant mid bf16 nf4 single[17] logit 5.2e-05 state 0.000112
  quant mid bf16 nf4 single[33] logit 7.62e-05 state 0.000159
  quant mid bf16 nf4 single[65] logit 5.79e-05 state 0.000174
  quant mid f16 int8 single[1] logit 2.27e-06 state 3.18e-06
  quant mid f16 int8 single[17] logit 5.84e-06 state 8.3e-06
  quant mid f16 int8 single[33] logit 3.41e-06 state 1.3e-05
  quant mid f16 int8 single[65] logit 3.97e-06 state 1.45e-05
  quant tiny bf16 int8 ragged logit 2.58e-05 state 0.000378
  quant tiny f16 int8 ragged logit 1.02e-06 state 1.66e-05
  quant tiny bf16 nf4 ragged logit 2.1e-05 state 0.000314
  quant tiny f16 nf4 ragged logit 1.05e-06 state 1.89e-05
  quant c384 bf16 int8 ragged logit 3.48e-05 state 0.000134
  quant c384 f16 nf4 ragged logit 1.87e-06 state 4.49e-06
  quant mid bf16 nf4 ragged logit 0.00021 state 0.000129
  quant mid f16 int8 ragged logit 3.3e-06 state 9.89e-06
  quant tiny bf16 int8 chunked logit 2.35e-05 state 0.000214
  quant tiny f16 int8 chunked logit 1.09e-06 state 1.46e-05
  quant tiny bf16 nf4 chunked logit 2.71e-05 state 0.000264
  quant tiny f16 nf4 chunked logit 1.44e-06 state 1.06e-05
  quant c384 bf16 int8 chunked logit 0.000123 state 0.00011
  quant c384 f16 nf4 chunked logit 1.85e-06 state 6.28e-06
  quant mid bf16 nf4 chunked logit 5.96e-05 state 0.000146
  quant mid f16 int8 chunked logit 3.55e-06 state 1.21e-05
  quant tiny f16 int8 small rows[1] logit 7.1e-07 state 6.7e-06
  quant tiny f16 int8 small rows[17] logit 1.55e-06 state 2.32e-05
  quant tiny f16 int8 uneven rows[1] logit 1.06e-06 state 7.67e-06
  quant tiny f16 int8 uneven rows[17] logit 2.33e-06 state 2.25e-05
  quant tiny f16 nf4 small rows[1] logit 8.01e-07 state 5.29e-06
  quant tiny f16 nf4 small rows[17] logit 2.98e-06 state 1.69e-05
  quant tiny f16 nf4 uneven rows[1] logit 1.54e-06 state 7.89e-06
  quant tiny f16 nf4 uneven rows[17] logit 9.94e-07 state 2.28e-05
and layer 0's WKV state in the shift cases (SHIFT-S0 lines of test_f16_shift):
  quant tiny f16 int8 small rows[1] layer-0 state: largest 3.17e-08, relative error 2.94e-07
  quant tiny f16 int8 small rows[17] layer-0 state: largest 1.09e-07, relative error 3.2e-07
  quant tiny f16 int8 uneven rows[1] layer-0 state: largest 0.0335, relative error 2.35e-07
  quant tiny f16 int8 uneven rows[17] layer-0 state: largest 0.114, relative error 2.68e-07
  quant tiny f16 nf4 small rows[1] layer-0 state: largest 2.94e-08, relative error 2.4e-07
  quant tiny f16 nf4 small rows[17] layer-0 state: largest 1.05e-07, relative error 3.6e-07
  quant tiny f16 nf4 uneven rows[1] layer-0 state: largest 0.0309, relative error 3.06e-07
  quant tiny f16 nf4 uneven rows[17] layer-0 state: largest 0.113, relative error 5.38e-07
"""
import functools

import numpy as np
import pytest

import quant_ref
import rwkv7_f64
import rwkvtts
from rwkvtts import weights as W
from forward_check import FULL, LAST, Reference, check_case, tokens

pytestmark = pytest.mark.gpu

V = 8209
HEAD = 200
STATE_GATE = 1e-3
DIMS = {"tiny": dict(W.DIMS_TINY, n_vocab=V), "c384": dict(W.DIMS_TINY, n_embd=384, n_ffn=1536, n_vocab=V),
        "mid": dict(W.DIMS_MID, n_vocab=V)}
QL = {"tiny": 2, "c384": 2, "mid": 1}
CASES = [("tiny", "bf16", "int8"), ("tiny", "f16", "int8"), ("tiny", "bf16", "nf4"), ("tiny", "f16", "nf4"),
         ("c384", "bf16", "int8"), ("c384", "f16", "nf4"), ("mid", "bf16", "nf4"), ("mid", "f16", "int8")]
SHIFT_CASES = [("tiny", "f16", qt, variant) for qt in ("int8", "nf4") for variant in ("small", "uneven")]
SPREAD_SCALE, SPREAD_EVERY, SPREAD_FACTOR = 4.0, 32, 16.0
# (the shift cases: layer 0 is scaled down and moves the logits less, so layer 1 takes a wider spread)
SHIFT_LAYER1 = (128, 64.0)
# What _spread's scales of k and v aim for: a float64 state no larger than this after the 64 probe tokens
# (the plain synthetic blobs reach 3.1 / 3.2 / 4.7 on tiny / c384 / mid; the blobs here 51 / 19 / 42, the
# shift cases 187). The state gate is absolute, 1e-3 ~ 2^-10. A bf16 engine's two planes carry an
# activation to 2^-16 .. 2^-17 of its size, so at 2^6 the gate is one such rounding of the largest entry;
# an f16 engine's planes carry 2^-22, so 2^8 leaves it 2^-18 / 2^-22 = 16 of them. A state larger than
# that would measure the reference's scale, not the kernels.
STATE_TOP = {"bf16": 64.0, "f16": 256.0}
SCALED = {"small": (quant_ref.TARGETS, -14), "uneven": ((W.L_WV, W.L_FFN_V), -8)}


def _scale_layer0(blob, dims, variant):
    """A copy of an f16 blob with `variant`'s matrices of layer 0 times 2^e, rounded to f16."""
    targets, e = SCALED[variant]
    out = blob.copy()
    for layer, t, off, rows, cols, _ in W.layout(dims)[0]:
        if layer == 0 and t in targets:
            m = out[off:off + 2 * rows * cols].view(np.float16)
            m[:] = np.ldexp(m.astype(np.float64), e).astype(np.float16)
            top = float(np.abs(m.astype(np.float64)).max())
            assert top > 0
            if variant == "small":  # shift_of: 14 - ceil(log2(top)) >= 25 before the clamp to 24
                assert top <= 2.0 ** -11, top
    return out


def _spread(blob, dims, dtype, n_layers, scale=SPREAD_SCALE, outliers=None):
    """A copy of a synthetic blob whose quantised matrices have a larger weight spread: every weight times `scale`
    (less for k and v, below), and every `every`-th weight of a row (from column row % every) times `factor` besides, all
    powers of two, so each product is exactly a number of the dtype. The synthetic weights (normal,
    sigma 0.02) fill a block's range so evenly that Int8 moves the logits by under one gate; an outlier
    per 32 weights widens every block's range sixteenfold and the scale raises the layers' share of the
    residual. `outliers`: {layer: (every, factor)} for layers that take another pair than
    (SPREAD_EVERY, SPREAD_FACTOR)."""
    out = blob.copy()
    for layer, t, off, rows, cols, _ in W.layout(dims)[0]:
        if 0 <= layer < n_layers and t in quant_ref.TARGETS:
            every, factor = (outliers or {}).get(layer, (SPREAD_EVERY, SPREAD_FACTOR))
            m = out[off:off + 2 * rows * cols].view(np.uint16).reshape(rows, cols)
            # (v k^T sets the WKV state's magnitude, which the absolute state gate assumes and a bf16 engine
            # follows to 2^-16 of it: k takes half the scale at C = 128 and k, v none at the wider sets)
            wide = dims["n_embd"] > 128
            x = quant_ref.decode(m, dtype).astype(np.float64) * (
                (1.0 if wide else scale / 2) if t == W.L_WK else 1.0 if wide and t == W.L_WV else scale)
            r, c = np.indices(x.shape)
            x[(c % every) == (r % every)] *= factor
            m[:] = quant_ref.encode(x, dtype)
    return out


@functools.lru_cache(maxsize=None)
def _case(name, dt, qt, variant=None):
    """(blob, Reference of the float64 quantised model, logit gate); asserts the 50-gate guard."""
    dims = DIMS[name]
    dtype = rwkvtts._ffi.DTYPE_F16 if dt == "f16" else rwkvtts._ffi.DTYPE_BF16
    blob = _spread(W.synth_blob(dims, seed=123, dtype=dtype), dims, dtype, QL[name],
                   outliers={1: SHIFT_LAYER1} if variant else None)
    if variant:
        blob = _scale_layer0(blob, dims, variant)
    ref = Reference(quant_ref.quantised_model(blob, dims, qt, QL[name]))
    probe = tokens(7, 64, V)
    quantised = ref.get(probe, V)[0]
    gate = 2e-3 * max(1.0, float(quantised.std()) / 1.6)
    st = (full := rwkv7_f64.Model(blob)).new_state()
    moved = np.abs(quantised - full.forward_rows(st, probe, V)).max()
    print(f"QUANT-GUARD {name} {dt} {qt} {variant or ''}: moved {moved:.3g} = {moved / gate:.0f} gates of {gate:.3g}")
    assert moved >= 50 * gate, (moved, gate)
    top = float(np.abs(ref.get(probe, V)[1]).max())
    print(f"QUANT-STATE {name} {dt} {qt} {variant or ''}: largest |state| {top:.3g}")
    assert top <= STATE_TOP[dt], top
    return blob, ref, gate


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    for e in _ENGINES.values():
        e.rt.close()
    _ENGINES.clear()
    _case.cache_clear()


class Eng:
    def __init__(self, name, dt, qt, variant=None, chunk=128):
        self.name, self.label = name, " ".join(x for x in ("quant", name, dt, qt, variant) if x)
        blob, self.ref, self.gate = _case(name, dt, qt, variant)
        self.rt = rwkvtts.SharedRwkvRuntime(blob, max_slots=4, token_chunk_size=chunk, use_graphs=False,
                                            quant_layers=QL[name], quant_type=qt)

    def check(self, inputs, case, **kw):
        return check_case(self.rt, self.ref, inputs, HEAD, self.gate, STATE_GATE, label=f"{self.label} {case}", **kw)


def _eng(case):
    """One engine per case for the whole module (token_chunk_size 128), closed when the module ends."""
    if case not in _ENGINES:
        _ENGINES[case] = Eng(*case)
    return _ENGINES[case]


IDS = ["-".join(c) for c in CASES]
# mid keeps 1 / 17 / 33 / 65: its float64 references and one-token-per-call runs cost the most
SINGLE = [(c, n) for c in CASES for n in (1, 16, 17, 32, 33, 65) if not (c[0] == "mid" and n in (16, 32))]


@pytest.mark.parametrize("case,n", SINGLE, ids=[f"{'-'.join(c)}-{n}" for c, n in SINGLE])
def test_single_segment(case, n):
    _eng(case).check([(tokens(200 + n, n, V), FULL, 2)], f"single[{n}]")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ragged_step(case):
    """Four slots with 5 / 16 / 23 / 1 rows in one call, the third with OPT_LAST."""
    opts = (FULL, FULL, LAST, FULL)
    _eng(case).check([(tokens(300 + i, n, V), o, i) for i, (n, o) in enumerate(zip((5, 16, 23, 1), opts))], "ragged")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chunked_prompt(case):
    """40 tokens through an engine with token_chunk_size 16: three calls of 16 / 16 / 8 tokens."""
    e = Eng(*case, chunk=16)
    try:
        e.check([(tokens(500, 40, V), FULL, 1)], "chunked", history=[[16], [16], [8]])
    finally:
        e.rt.close()


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("case", SHIFT_CASES, ids=["-".join(c) for c in SHIFT_CASES])
def test_f16_shift(case, n):
    e, toks = _eng(case), tokens(600 + n, n, V)
    e.check([(toks, FULL, 2)], f"rows[{n}]")
    # Layer 0's WKV state S = sum v k^T is what is left of its scaled matrices that can be measured: with
    # wk and wv 2^-14 (small) or wv 2^-8 (uneven) lower it is far below the absolute state gate, so it is
    # compared RELATIVE to its own largest entry, with the state gate's figure (1e-3). A shift applied off
    # by one bit in the rkv launch doubles or halves it, and dropped codes zero it: 1000 bounds either way.
    # (Wo and the FFN of a layer scaled by 2^-14 reach neither state nor logits above 1e-6: for `small`
    # their launches' clamped shift is held by the bitwise assertions and the absence of Inf / NaN only.)
    m = e.ref.model
    lo, hi = m.C, m.C + m.H * m.N * m.N
    want = e.ref.get(toks, HEAD)[1][lo:hi]
    got = e.rt.read_slot(2)[lo:hi]
    top = np.abs(want).max()
    assert np.isfinite(got).all() and top > 2.0 ** -100
    rel = np.abs(got - want).max() / top
    print(f"SHIFT-S0 {e.label} rows[{n}] layer-0 state: largest {top:.3g}, relative error {rel:.3g}")
    assert rel < STATE_GATE, rel
