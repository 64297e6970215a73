"""The LM forward pass at ragged steps and tile edges, at the 0.4B widths (DIMS_MID, n_vocab 77923).

Every step is ONE rt.infer call whose inputs all ask for every row's logits (OPT_FULL), on engines
with use_graphs=False and max_slots=8: bf16 and f16, and for the 128-token engine also one created
with wkv_variant=1 (id bf16_wkv4; the engine ignores the field). Tokens are uniform random ids
below n_vocab from fixed seeds. Every case makes the three assertions of forward_check.check_case:
float64 reference (logits < 2e-3, state < 1e-3: test_gpu_forward.py's bounds, now against an exact
reference), bitwise equality with the segment run alone, bitwise equality with one token per call
(the header's "outputs are chunk-invariant").

What each case crosses (R = rows of the step, mg = ceil(R / 32) row groups):

  single segments, token_chunk_size 128
    1            R == n_seg: the one-row WKV kernel, mt = 1 (launch_gemm: M <= 16)
    2, 15, 16    mt = 1 up to 16 rows; one partly filled / one full WKV chunk (kRowsChunk 16); 15 is
                 an odd count, so the last kRowsGroup pair re-reads its last row (min(gi, nr - g0 - 1))
    17           mt = 2 from 17 rows; a second WKV chunk of one row
    31, 33       one 32-row group partly filled; a second group of one row, a third WKV chunk
    47, 49       odd row counts across three / four WKV chunks
    63, 64, 65   kPlaneRows = 64 (engine.hip): <= 64 rows stage relu^2 inside the value GEMM
                 (kXRelu2, NX 4), 65 rows run k_relu2_planes + a planes-mode value GEMM (bf16
                 engines; f16 engines have no planes buffers and keep kXRelu2). 65 = 2 groups + 1 row
  ragged, same engines, slots out of ascending order
    [1, 17, 2, 33, 1, 16, 3]   one-row segments beside long ones in one multi-row launch (wkv6_rows
                 with n_rows = 1), segments starting at rows that are no multiple of 16 or 32
    [15, 1, 1, 1]   R = 18 > n_seg = 4: multi-row launch, mostly one-row segments, mt = 2
    [5] * 8      all eight slots, R = 40
    [64, 1]      R = 65: the planes route with a one-row segment in the last, one-row group
  large, token_chunk_size 640, head_rows 100: launch_gemm_t gives a workgroup rpw row groups,
  rpw = max(1, mg * tiles * k_split / 1024) (k_gemm_wide: tiles / 2), grid.z = ceil(mg / rpw):

      R    mg | rkv (53 x 4) | Wo (16 x 8) | key, wide (32 x 4) | value bf16, wide (8 x 16) | value f16 (16 x 16)
     300   10 |  2 -> 5      |  1 -> 10    |  1 -> 10           |  1 -> 10                  |  2 -> 5
     353   12 |  2 -> 6      |  1 -> 12    |  1 -> 12           |  1 -> 12                  |  3 -> 4
     511   16 |  3 -> 6 (1)  |  2 -> 8     |  2 -> 8            |  2 -> 8                   |  4 -> 4
     577   19 |  3 -> 7 (1)  |  2 -> 10 (1)|  2 -> 10 (1)       |  2 -> 10 (1)              |  4 -> 5 (3)

    ("3 -> 7 (1)": rpw 3, 7 workgroups along z, the last one holding 1 group.) rkv and the f16
    value GEMM are k_gemm2 (KSTEPS 8), Wo is k_gemm2 with KSTEPS 4, the key GEMM and the bf16
    value GEMM (planes) are k_gemm_wide. 353 and 577 end in a one-row group; at 577 the group count
    19 is a multiple of no launch's rpw, so every form's last workgroup gets a short share. The
    head GEMM (2 tiles x 2 splits) keeps rpw = 1 throughout.
  budget cuts, token_chunk_size 64 (Engine::infer)
    40 / 40 / 40 -> consumed 40 / 24 / 0, then 0 / 16 / 40: an input cut short, an input given no
    rows, then an emptied input in front of the others; [10, 0, 20]: n_tokens = 0 in the middle;
    OPT_LAST between two OPT_FULL inputs: n_lg != R, ln_out through row_map; OPT_LAST cut short
    (no logits in the first call, its last row's in the second)
  head edge, 3 rows: head_rows 1, 15, 17, 63, 65 (the first 64-column tile partly filled / just
    exceeded), 77923 (Vpad = 77936: the last of 1218 tiles holds 35 columns)
  hand-over: a ragged step, a step of one row per slot (R == n_seg: the one-row WKV kernel reads
    the state wkv6_rows wrote), a second ragged step, then every slot's state
"""
import functools

import numpy as np
import pytest

import rwkvtts
from rwkvtts import weights as W

import rwkv7_f64
from forward_check import FULL, LAST, Reference, check_case, feed, tokens

pytestmark = pytest.mark.gpu

LOGIT_GATE = 2e-3  # test_gpu_forward.LOGIT_ATOL
STATE_GATE = 1e-3
V = W.DIMS_MID["n_vocab"]


@functools.lru_cache(maxsize=None)
def _model(dt):
    """(blob, float64 reference) of DIMS_MID for a dtype: built once per module run."""
    dtype = rwkvtts._ffi.DTYPE_F16 if dt == "f16" else rwkvtts._ffi.DTYPE_BF16
    blob = W.synth_blob(W.DIMS_MID, seed=123, dtype=dtype)
    return blob, Reference(rwkv7_f64.Model(blob))


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _model.cache_clear()  # two 330 MB blobs and their references


def _engine(param, chunk):
    dt, _, variant = param.partition("_")
    blob, ref = _model(dt)
    rt = rwkvtts.SharedRwkvRuntime(blob, max_slots=8, token_chunk_size=chunk, use_graphs=False,
                                   wkv_variant=1 if variant == "wkv4" else 0)
    return rt, ref


@pytest.fixture(scope="module", params=["bf16", "f16", "bf16_wkv4"])
def eng128(request):
    rt, ref = _engine(request.param, 128)
    yield rt, ref, request.param
    rt.close()


@pytest.fixture(scope="module", params=["bf16", "f16"])
def eng640(request):
    rt, ref = _engine(request.param, 640)
    yield rt, ref, request.param
    rt.close()


@pytest.fixture(scope="module", params=["bf16", "f16"])
def eng64(request):
    rt, ref = _engine(request.param, 64)
    yield rt, ref, request.param
    rt.close()


def _inputs(seed, lens, slots, options=None):
    return [(tokens(1000 * seed + i, n, V), options[i] if options else FULL, s)
            for i, (n, s) in enumerate(zip(lens, slots))]


def _check(eng, inputs, head_rows, label, **kw):
    rt, ref, name = eng
    return check_case(rt, ref, inputs, head_rows, LOGIT_GATE, STATE_GATE, label=f"mid {name} {label}", **kw)


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 33, 47, 49, 63, 64, 65])
def test_single_segment(eng128, n):
    _check(eng128, _inputs(n, [n], [3]), 200, f"single[{n}]")


RAGGED = {"mixed": ([1, 17, 2, 33, 1, 16, 3], [5, 0, 3, 7, 1, 6, 2]),
          "ones": ([15, 1, 1, 1], [2, 7, 0, 4]),
          "eight": ([5] * 8, [3, 0, 6, 1, 7, 2, 5, 4]),
          "planes": ([64, 1], [6, 1])}


@pytest.mark.parametrize("case", sorted(RAGGED))
def test_ragged_step(eng128, case):
    lens, slots = RAGGED[case]
    _check(eng128, _inputs(100 + len(lens), lens, slots), 200, f"ragged[{case}]")


LARGE = {300: [137, 163], 353: [200, 1, 152], 511: [255, 256], 577: [300, 33, 244]}


@pytest.mark.parametrize("R", sorted(LARGE))
def test_large_step(eng640, R):
    lens = LARGE[R]
    assert sum(lens) == R
    _check(eng640, _inputs(R, lens, [4, 1, 6][:len(lens)]), 100, f"large[{R}]")


def test_budget_cuts_an_input_short(eng64):
    _check(eng64, _inputs(40, [40, 40, 40], [2, 5, 0]), 200, "budget[40,40,40]",
           history=[[40, 24, 0], [0, 16, 40]])


def test_empty_input_among_others(eng64):
    _check(eng64, _inputs(41, [10, 0, 20], [6, 3, 1]), 200, "budget[10,0,20]")


def test_last_beside_full(eng64):
    _check(eng64, _inputs(42, [12, 9, 20], [1, 7, 4], [FULL, LAST, FULL]), 200, "budget[full,last,full]")


def test_last_cut_short(eng64):
    _check(eng64, _inputs(43, [40, 40, 40], [3, 0, 6], [FULL, LAST, FULL]), 200, "budget[40,last 40,40]",
           history=[[40, 24, 0], [0, 16, 40]])


@pytest.mark.parametrize("head_rows", [1, 15, 17, 63, 65, V])
def test_head_edge(eng128, head_rows):
    _check(eng128, _inputs(50, [3], [2]), head_rows, f"head[{head_rows}]")


def test_hand_over_between_wkv_kernels(eng128):
    rt, ref, name = eng128
    slots = [4, 1, 6, 2]
    parts = [[3, 17, 1, 20], [1, 1, 1, 1], [16, 2, 33, 5]]
    for s in slots:
        rt.reset_slot(s)
    got, toks = [[] for _ in slots], [[] for _ in slots]
    for p, lens in enumerate(parts):
        step = _inputs(60 + p, lens, slots)
        out, calls, _ = feed(rt, step, 200)
        assert calls == 1
        for i in range(len(slots)):
            got[i].append(out[i])
            toks[i] += step[i][0]
    inputs = [(t, FULL, s) for t, s in zip(toks, slots)]
    check_case(rt, ref, inputs, 200, LOGIT_GATE, STATE_GATE, got=[np.vstack(g) for g in got],
               label=f"mid {name} hand-over")
