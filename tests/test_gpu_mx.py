"""Microscaling weights (RWKVTTS_QUANT_MXFP8 / MXFP4, include/rwkvtts.h) on the GPU.

A dequantised MX weight is exactly a bf16 number, so an engine with MX layers must equal, bit for bit,
an unquantised engine on a blob whose quantised matrices hold tests/mx_ref.py's dequantised values:
the quantisation rule is checked through rwkvtts_mx_roundtrip, the GEMM (k_gemm_mx) through logits and
slot state. mid (C = 1024) has the 256-deep K-slices and split-K of the 0.4B model, c384 key split 3
(summed slab up to 64 rows, relu^2 planes beyond); a 70-row step is past the 64-row switch."""
import numpy as np
import pytest

import mx_ref
import rwkvtts
from rwkvtts import weights as W
from forward_check import FULL, tokens
from helpers import make_request, synth_text, to_struct

pytestmark = pytest.mark.gpu

LOGIT_ATOL = 2e-3  # as tests/test_gpu_quant.py
HEAD = 8193
DIMS = {"tiny": W.DIMS_TINY, "small": W.DIMS_SMALL, "mid": W.DIMS_MID,
        "c384": dict(W.DIMS_TINY, n_embd=384, n_ffn=1536)}
CASES = [("tiny", "mxfp4", 2), ("small", "mxfp8", 3), ("mid", "mxfp4", 1), ("c384", "mxfp8", 2)]


def _roundtrip_matrix(fmt):
    """16 x 128 bf16 bits: the blocks the contract's edges need, at three block scales."""
    emax, mbits, emin_el, sat, _ = mx_ref.FORMATS[fmt]
    top, ulp = 2.0 ** emax, 2.0 ** (emax - mbits)
    mids = [1 + (2 * i + 1) * 2.0 ** -(mbits + 1) for i in range(2 ** mbits)]  # element midpoints in [1, 2): ties both ways
    subs = [(2 * i + 1) * 2.0 ** (emin_el - mbits - 1) for i in range(2 ** mbits)]  # midpoints among the subnormals
    tiny = 2.0 ** -126  # the smallest dequantised magnitude of either type
    blocks = []
    for s in (1.0, 2.0 ** -20, 2.0 ** 90):
        blocks.append([s * x for x in [top] + mids + [-m for m in subs] + [top / 2 * m for m in mids]])  # amax = 2^n
        blocks.append([s * x for x in [2 * top * (1 - 2.0 ** -8)] + mids])                # amax just below 2^(n + 1)
        blocks.append([s * x for x in [sat + ulp / 2, sat + ulp, -(sat + 1.5 * ulp), sat - ulp / 2]])  # past saturation
    blocks.append([0.0, -0.0])                                                            # all zero, one -0
    blocks.append([tiny * x for x in (3, 0.5, -0.5, 1.5, 2.5, 1)])                        # amax under the exponent clamp
    blocks.append([float(W.bf16_bits_to_f32(np.uint16(0x7F7F))), 1.0, -1.5 * 2.0 ** 127, 1.5 * 2.0 ** 119])  # the largest finite bf16
    m = np.zeros((64, 32), np.float64)
    for i in range(64):
        b = blocks[i % len(blocks)]
        m[i, :len(b)] = b if i < len(blocks) else b[::-1]
    f = m.astype(np.float32)
    assert (f.astype(np.float64) == m).all() and not (f.view(np.uint32) & 0xFFFF).any(), "not bf16 numbers"
    return (f.view(np.uint32) >> 16).astype(np.uint16).reshape(16, 128)


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_roundtrip(fmt):
    w = _roundtrip_matrix(fmt)
    got, want = rwkvtts.runtime.mx_roundtrip(fmt, w), mx_ref.dequantised(w, fmt)
    bad = np.argwhere(got != want)
    assert not len(bad), [(hex(w[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]]


@pytest.fixture(scope="module", params=CASES, ids=["-".join(map(str, c)) for c in CASES])
def pair(request):
    """(dims, dequantised blob, MX engine on the original blob, unquantised engine on the dequantised one)"""
    name, fmt, ql = request.param
    dims = DIMS[name]
    blob = W.synth_blob(dims, seed=321)
    deq = mx_ref.dequantised_blob(blob, dims, fmt, ql)
    assert not np.array_equal(blob, deq)
    kw = dict(max_slots=4, token_chunk_size=128, use_graphs=True)
    rt_mx = rwkvtts.SharedRwkvRuntime(blob, quant_layers=ql, quant_type=fmt, **kw)
    rt_16 = rwkvtts.SharedRwkvRuntime(deq, **kw)
    yield dims, deq, rt_mx, rt_16
    rt_mx.close()
    rt_16.close()


def _run(rt, slots, parts):
    """parts: per call, one token list per slot. Returns every call's logits and the final states."""
    for s in slots:
        rt.reset_slot(s)
    outs = []
    for part in parts:
        _, out = rt.infer(rwkvtts.RnnInput([rwkvtts.RnnInputBatch(list(p), FULL) for p in part], 128),
                          head_rows=HEAD, slots=slots)
        assert [o.shape for o in out] == [(len(p), HEAD) for p in part]
        outs += out
    return np.concatenate(outs), [rt.read_slot(s) for s in slots]


def test_forward_bitwise(pair):
    dims, _, rt_mx, rt_16 = pair
    toks = tokens(9, 70, dims["n_vocab"])
    steps = [[[toks[4 * i + s]] for s in range(4)] for i in range(3)]  # one-token steps, 4 slots together
    for slots, parts in (([0], [[toks]]), ([1], [[toks[:35]], [toks[35:]]]), ([0, 1, 2, 3], steps)):
        got, st = _run(rt_mx, slots, parts)
        want, st_want = _run(rt_16, slots, parts)
        assert np.array_equal(got, want), (slots, np.abs(got - want).max())
        assert all(np.array_equal(a, b) for a, b in zip(st, st_want)), slots


def test_oracle_and_tokens(pair):
    dims, deq, rt_mx, _ = pair
    import oracle
    om = oracle.Model(deq)
    toks = tokens(9, 20, dims["n_vocab"])
    st = om.new_state()
    ref = np.stack([om.forward(st, t, HEAD) for t in toks])
    got, _ = _run(rt_mx, [0], [[toks]])
    assert np.abs(got - ref).max() < LOGIT_ATOL, np.abs(got - ref).max()
    reqs = [make_request(synth_text(500 + i), seed=700 + i, fixed=20) for i in range(3)]
    for r, (g, s) in zip(reqs, rt_mx.generate_batch(reqs)):
        q, keep = to_struct(r)
        og, os_, _ = om.generate(q)
        assert (g, s) == (og, os_)


def test_f16_refused():
    blob = W.synth_blob(W.DIMS_TINY, seed=1, dtype=rwkvtts._ffi.DTYPE_F16)
    with pytest.raises(rwkvtts._ffi.RwkvTtsError) as e:
        rwkvtts.SharedRwkvRuntime(blob, max_slots=2, quant_layers=1, quant_type="mxfp4")
    assert e.value.code == rwkvtts._ffi.EUNSUPPORTED and "f16" in str(e.value)
