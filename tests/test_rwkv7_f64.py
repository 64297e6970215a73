"""tests/rwkv7_f64.py (the float64 restatement the GPU shape and dims tests measure against) vs the
C oracle: 97 uniformly random tokens from a zero state, every row's logits and the final state.

The difference is the oracle's own f32 rounding, which grows with C. Measured with a per-token
float64 prototype (bf16, seed 123): logits 1.5e-6 / 8.3e-6 / 1.4e-5 / 2.7e-5 and state 7.6e-7 /
2.4e-6 / 4.5e-6 / 1.4e-5 at C = 128 / 768 / 1024 / 2048. The gates are about 7 times the worst of
those: a restatement that differs from the oracle in a formula, not in rounding, misses them by
orders of magnitude.
"""
import numpy as np
import pytest

import rwkvtts
from rwkvtts import weights as W

import rwkv7_f64

LOGIT_GATE = 2e-4
STATE_GATE = 1e-4
HEAD_ROWS = 8193
N_TOKENS = 97

DIMS_C128X = dict(n_layer=3, n_embd=128, head_size=64, n_ffn=384, n_vocab=8209,
                  d_decay=16, d_aaa=32, d_mv=16, d_gate=16)
DIMS_C768 = dict(n_layer=2, n_embd=768, head_size=64, n_ffn=3072, n_vocab=8209,
                 d_decay=64, d_aaa=64, d_mv=32, d_gate=128)
DIMS_C2048 = dict(n_layer=2, n_embd=2048, head_size=64, n_ffn=4096, n_vocab=8209,
                  d_decay=96, d_aaa=96, d_mv=64, d_gate=256)

BF16, F16 = rwkvtts._ffi.DTYPE_BF16, rwkvtts._ffi.DTYPE_F16


def _check(dims, dtype, oracle_mod):
    blob = W.synth_blob(dims, seed=123, dtype=dtype)
    om = oracle_mod.Model(blob)
    fm = rwkv7_f64.Model(blob)
    toks = np.random.RandomState(97).randint(0, dims["n_vocab"], size=N_TOKENS).tolist()
    st = om.new_state()
    ref = np.stack([om.forward(st, t, HEAD_ROWS) for t in toks])
    st64 = fm.new_state()
    assert st64.size == st.size
    # two calls: the second starts from a non-zero state and a non-zero shift row
    got = np.vstack([fm.forward_rows(st64, toks[:40], HEAD_ROWS), fm.forward_rows(st64, toks[40:], HEAD_ROWS)])
    assert got.shape == ref.shape and got.dtype == np.float64
    lerr, serr = np.abs(got - ref).max(), np.abs(st64 - st).max()
    print(f"C={dims['n_embd']} dtype={dtype}: logit {lerr:.3g} state {serr:.3g}")
    assert lerr < LOGIT_GATE, lerr
    assert serr < STATE_GATE, serr


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("dims", [DIMS_C128X, DIMS_C768], ids=["c128x", "c768"])
def test_f64_matches_oracle(dims, dtype, oracle_mod):
    _check(dims, dtype, oracle_mod)


@pytest.mark.parametrize("dims", [W.DIMS_MID, DIMS_C2048], ids=["mid", "c2048"])
def test_f64_matches_oracle_wide(dims, oracle_mod):
    """The widest sets, bf16 only (2 to 3 s each with the batched form: not marked slow)."""
    _check(dims, BF16, oracle_mod)


def test_numpy_blob_decodes_the_same():
    """The independent numpy generator's blob gives the same model as the library's."""
    a = rwkv7_f64.Model(W.synth_blob(DIMS_C128X, seed=123))
    b = rwkv7_f64.Model(W.synth_blob_numpy(DIMS_C128X, seed=123))
    sa, sb = a.new_state(), b.new_state()
    toks = [5, 8208, 0, 77]
    assert np.array_equal(a.forward_rows(sa, toks, 17), b.forward_rows(sb, toks, 17))
    assert np.array_equal(sa, sb)
