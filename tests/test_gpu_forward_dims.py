"""The LM forward pass at dims Engine::init admits and no other test runs.

Three sets, each with n_vocab = 8209 (no multiple of 16: Vpad = 8224 != n_vocab, and the last of
the head GEMM's 129 column tiles holds 17 columns), bf16 and f16, use_graphs=False, max_slots=8:

  set     dims                                             split-K (rkv / Wo / key / value / head)
  c128x   L=3 C=128  F=384  ranks 16/32/16/16   H=2        1 / 1 / 1 / 3 / 1
  c768    L=2 C=768  F=3072 ranks 64/64/32/128  H=12       3 / 6 / 3 / 12 / 3
  c2048   L=2 C=2048 F=4096 ranks 96/96/64/256  H=32       8 / 16 / 8 / 16 / 4

Where they land (Engine::init's pick(); launch_wkv, launch_ln_mix, launch_gemm_t):

  launch_wkv     units = ceil(rank total / 16), n_part = the rkv split. c128x: 5 units, 1 slab, and
                 ranks that are not k_wkv2's 16/16/16/32 -> k_wkv<8,4>. c768: 18 units, 3 slabs (the
                 0.4B ranks, but not its 4 slabs, so not k_wkv6) -> k_wkv<20,4>. c2048:
                 32 units, 8 slabs -> k_wkv<32,8>.
  launch_ln_mix  C != 1024, so never k_ln1024. c128x and c768: k_ln_mix<1,0> (layer 0) and
                 k_ln_mix<1,-1> with 3 / 1 and 12 / 6 slabs (LN1 of layers > 0 and ln_out sum the
                 value split's slabs, LN2 the Wo split's). c2048: C > 1024 -> k_ln_mix<2,-1>
                 (16 / 16 slabs).
  launch_gemm_t  the value GEMM's fused relu^2 staging has k_gemm2 forms for 1, 2 and 4 key slabs:
                 c128x (key split 1) stages its one slab; c768 (3) and c2048 (8) sum their slabs into
                 slab 0 first (k_sum_slabs) and stage that, at <= 64 rows on bf16 engines and at every
                 row count on f16 engines (no relu^2 planes). The planes-mode GEMMs (rkv, Wo, key,
                 head; the bf16 value GEMM above 64 rows) are k_gemm2 / k_gemm_wide with kslice
                 128 / 256.
  grids          the XCD-mapped 1-D grids (kXmapMask: value GEMM and WKV) exist in k_gemm2 and
                 k_wkv6 only and need a split that divides 8 or is a multiple of it: c2048's fused
                 value GEMM (split 16) takes the 1-D grid in steps of one row group; c128x (3) and
                 c768 (12; H = 12, splits 3 / 6 / 12) keep the plain (tiles, k_split, mg) grid, and
                 every WKV launch the (n_seg, H) grid. The key GEMM's XCD-aligned grid (kXalignMask, steps of <= 32 rows) pads
                 its tile groups to a multiple of 8: c128x has 3 groups of 2 tiles (-> 8), c768 12
                 groups of 4 (-> 16); the 0.4B widths have 16 and never pad.

Per set and dtype: the four tests of test_gpu_forward.py (reference with per-row logits, eight
teacher-forced decode steps and the state; 7-token chunks bitwise; batch invariance bitwise; state
round trip) and a reduced shape sweep with forward_check.check_case's three assertions (float64,
bitwise segment alone, bitwise one token per call).

Logit gate: 2e-3 * max(1, sigma / 1.6), sigma the standard deviation of the float64 reference's
logits for the set, 1.6 the logit scale test_gpu_forward.py states its 2e-3 at. State gate 1e-3.

test_c768_decode_graph: c768 at n_vocab 77923 with graphs on. The persistent attention launch is
not tried (it needs layer 0's embedding fusion, C = 1024) and the persistent FFN launch declines the
shape at layer 0 (prep_ffn_persist: C != 1024), so every decode step runs the separate launches
inside a captured graph; tokens must equal the oracle's.
"""
import functools

import numpy as np
import pytest

import rwkvtts
from rwkvtts import weights as W

import rwkv7_f64
from forward_check import FULL, Reference, check_case, feed, tokens
from helpers import make_request, synth_text, to_struct

pytestmark = pytest.mark.gpu

V = 8209
DIMS = {
    "c128x": dict(n_layer=3, n_embd=128, head_size=64, n_ffn=384, n_vocab=V,
                  d_decay=16, d_aaa=32, d_mv=16, d_gate=16),
    "c768": dict(n_layer=2, n_embd=768, head_size=64, n_ffn=3072, n_vocab=V,
                 d_decay=64, d_aaa=64, d_mv=32, d_gate=128),
    "c2048": dict(n_layer=2, n_embd=2048, head_size=64, n_ffn=4096, n_vocab=V,
                  d_decay=96, d_aaa=96, d_mv=64, d_gate=256),
}
STATE_GATE = 1e-3


@functools.lru_cache(maxsize=None)
def _model(name, dt):
    dtype = rwkvtts._ffi.DTYPE_F16 if dt == "f16" else rwkvtts._ffi.DTYPE_BF16
    blob = W.synth_blob(DIMS[name], seed=123, dtype=dtype)
    ref = Reference(rwkv7_f64.Model(blob))
    sigma = float(ref.get(tokens(7, 64, V), V)[0].std())
    return blob, ref, 2e-3 * max(1.0, sigma / 1.6)


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _model.cache_clear()


class Eng:
    def __init__(self, name, dt):
        self.label = f"{name} {dt}"
        blob, self.ref, self.gate = _model(name, dt)
        self.rt = rwkvtts.SharedRwkvRuntime(blob, max_slots=8, token_chunk_size=128, use_graphs=False)

    def check(self, inputs, head_rows, case):
        return check_case(self.rt, self.ref, inputs, head_rows, self.gate, STATE_GATE, label=f"{self.label} {case}")


@pytest.fixture(scope="module", params=[f"{n}-{dt}" for n in DIMS for dt in ("bf16", "f16")])
def eng(request):
    e = Eng(*request.param.split("-"))
    yield e
    e.rt.close()


def _one(rt, toks, slot, head_rows, option=FULL):
    _, out = rt.infer(rwkvtts.RnnInput([rwkvtts.RnnInputBatch(list(toks), option)], 128), head_rows=head_rows,
                      slots=[slot])
    return out[0]


def test_prefill_and_decode_logits(eng):
    rt = eng.rt
    toks = tokens(1, 32, V)
    more = tokens(2, 8, V)
    want, st = eng.ref.get(toks + more, V)
    rt.reset_slot(0)
    got = _one(rt, toks, 0, V)
    assert got.shape == (32, V)
    lerr = np.abs(got - want[:32]).max()
    _, st32 = eng.ref.get(toks, 1)
    serr = np.abs(rt.read_slot(0) - st32).max()
    for i, t in enumerate(more):  # teacher-forced decode, OPT_LAST
        o = _one(rt, [t], 0, V, rwkvtts.RnnOption.Last)
        lerr = max(lerr, np.abs(o - want[32 + i]).max())
    serr = max(serr, np.abs(rt.read_slot(0) - st).max())
    print(f"FWD-ERR {eng.label} prefill+decode logit {lerr:.3g} state {serr:.3g} (gate {eng.gate:.3g})")
    assert lerr < eng.gate, lerr
    assert serr < STATE_GATE, serr


def test_chunked_prefill_is_bitwise_identical(eng):
    rt = eng.rt
    toks = tokens(3, 32, V)
    rt.reset_slot(1)
    full = _one(rt, toks, 1, 4096, rwkvtts.RnnOption.Last)
    rt.reset_slot(2)
    for i in range(0, len(toks), 7):
        out = _one(rt, toks[i:i + 7], 2, 4096, rwkvtts.RnnOption.Last)
    assert np.array_equal(out, full)
    assert np.array_equal(rt.read_slot(1), rt.read_slot(2))


def test_batch_invariance(eng):
    """A slot's logits do not depend on which other slots share the step."""
    rt = eng.rt
    prompts = [tokens(10 + i, 32, V) for i in range(4)]
    for s in range(5):
        rt.reset_slot(s)
    together, calls, _ = feed(rt, [(p, rwkvtts.RnnOption.Last, s) for s, p in enumerate(prompts)], 8193)
    assert calls == 1
    for s in range(4):
        rt.reset_slot(4)
        alone = _one(rt, prompts[s], 4, 8193, rwkvtts.RnnOption.Last)
        assert np.array_equal(alone, together[s][0]), s
        assert np.array_equal(rt.read_slot(4), rt.read_slot(s)), s


def test_state_roundtrip(eng):
    rt = eng.rt
    rt.reset_slot(0)
    _one(rt, tokens(4, 32, V), 0, 16, rwkvtts.RnnOption.Last)
    s = rt.read_slot(0)
    rt.write_slot(5, s)
    assert np.array_equal(rt.read_slot(5), s)
    a = _one(rt, [100], 0, 4096, rwkvtts.RnnOption.Last)
    b = _one(rt, [100], 5, 4096, rwkvtts.RnnOption.Last)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [1, 16, 17, 33, 65])
def test_single_segment(eng, n):
    """1: the one-row launch; 16 / 17: mt 1 -> 2 and the WKV kernels' row loop; 33: a second 32-row
    group of one row; 65: past kPlaneRows (bf16: k_relu2_planes + planes-mode value GEMM)."""
    eng.check([(tokens(200 + n, n, V), FULL, 3)], 200, f"single[{n}]")


def test_ragged_step(eng):
    lens, slots = [1, 17, 2, 33], [5, 0, 7, 2]
    eng.check([(tokens(300 + i, n, V), FULL, s) for i, (n, s) in enumerate(zip(lens, slots))], 200, "ragged")


@pytest.mark.parametrize("head_rows", [17, 8193, V])
def test_head_rows(eng, head_rows):
    """17: one partly filled tile; 8193 = 128 tiles + 1 column; 8209: the whole vocabulary, whose
    last tile ends inside the Vpad padding."""
    eng.check([(tokens(400, 3, V), FULL, 6)], head_rows, f"head[{head_rows}]")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_c768_decode_graph(dt):
    dtype = rwkvtts._ffi.DTYPE_F16 if dt == "f16" else rwkvtts._ffi.DTYPE_BF16
    blob = W.synth_blob(dict(DIMS["c768"], n_vocab=77923), seed=5, dtype=dtype)
    import oracle
    om = oracle.Model(blob)
    rt = rwkvtts.SharedRwkvRuntime(blob, max_slots=4, token_chunk_size=128, use_graphs=True)
    try:
        reqs = [make_request(synth_text(400 + i), seed=600 + i, fixed=12) for i in range(3)]
        got = rt.generate_batch(reqs)
        for r, (g, s) in zip(reqs, got):
            q, _keep = to_struct(r)
            og, os_, _ = om.generate(q)
            assert (g, s) == (og, os_)
    finally:
        rt.close()
