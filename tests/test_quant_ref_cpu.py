"""tests/quant_ref.py (the numpy restatement of RWKVTTS_QUANT_INT8 / NF4 that the GPU tests measure
against) tied to the reference the project already trusts, with no kernel involved:

* the float64 quantised model against oracle.Model(blob, quant_layers, quant_type) on DIMS_TINY. The
  difference is the oracle's own f32 rounding; the gates are tests/test_rwkv7_f64.py's rule, 7 times
  what that file measured for the unquantised pair at C = 128 (logits 1.5e-6, state 7.6e-7). One code
  that differs moves a weight by a whole quantisation step, orders of magnitude more;
* the exact (fractions) and the vectorised (numpy float32) forms agree bit for bit on the edge matrix
  of test_gpu_quant.py::test_roundtrip, whose edges are asserted present here as there.
"""
import numpy as np
import pytest

import quant_ref
import rwkvtts
from rwkvtts import weights as W

LOGIT_GATE = 7 * 1.5e-6
STATE_GATE = 7 * 7.6e-7
BF16, F16 = rwkvtts._ffi.DTYPE_BF16, rwkvtts._ffi.DTYPE_F16
COMBOS = [(qt, dt) for qt in ("int8", "nf4") for dt in (BF16, F16)]
IDS = [f"{qt}-{'bf16' if dt == BF16 else 'f16'}" for qt, dt in COMBOS]


@pytest.mark.parametrize("qt,dtype", COMBOS, ids=IDS)
def test_quantised_model_matches_oracle(qt, dtype, oracle_mod):
    dims = W.DIMS_TINY
    blob = W.synth_blob(dims, seed=321, dtype=dtype)
    toks = np.random.RandomState(11).randint(0, dims["n_vocab"], size=24).tolist()
    for ql in (1, 2):
        om = oracle_mod.Model(blob, quant_layers=ql, quant_type=rwkvtts.runtime.parse_quant_type(qt))
        st = om.new_state()
        ref = np.stack([om.forward(st, t, 1024) for t in toks])
        fm = quant_ref.quantised_model(blob, dims, qt, ql)
        st64 = fm.new_state()
        got = fm.forward_rows(st64, toks, 1024)
        lerr, serr = np.abs(got - ref).max(), np.abs(st64 - st).max()
        print(f"{qt} dtype={dtype} layers={ql}: logit {lerr:.3g} state {serr:.3g}")
        assert lerr < LOGIT_GATE, lerr
        assert serr < STATE_GATE, serr


@pytest.mark.parametrize("qt,dtype", COMBOS, ids=IDS)
def test_exact_and_vectorised_agree_on_the_edge_matrix(qt, dtype):
    bits, edges = quant_ref.edge_matrix(dtype, qt)
    assert bits.shape == (16, 256) and np.isfinite(quant_ref.decode(bits, dtype)).all()
    ex = quant_ref.exact(bits, dtype, qt)
    quant_ref.assert_edges(bits, dtype, qt, edges, ex)
    fast = quant_ref.dequantised(bits, dtype, qt).astype(np.float32)
    bad = np.argwhere(fast.view(np.uint32) != ex["w"].view(np.uint32))
    assert not len(bad), [(int(r), int(c), hex(bits[r, c]), float(fast[r, c]), float(ex["w"][r, c])) for r, c in bad[:8]]


def test_dequantised_weights_of_a_synthetic_matrix():
    """On ordinary weights too (one r matrix of each dtype): exact and vectorised forms, bit for bit."""
    for dtype in (BF16, F16):
        blob = W.synth_blob(W.DIMS_TINY, seed=321, dtype=dtype)
        layer, t, off, rows, cols, _ = next(e for e in W.layout(W.DIMS_TINY)[0] if e[0] == 0 and e[1] == W.L_WR)
        m = blob[off:off + 2 * rows * cols].view(np.uint16).reshape(rows, cols)[:16]
        for qt in ("int8", "nf4"):
            fast = quant_ref.dequantised(m, dtype, qt).astype(np.float32)
            assert np.array_equal(fast.view(np.uint32), quant_ref.exact(m, dtype, qt)["w"].view(np.uint32)), (dtype, qt)
