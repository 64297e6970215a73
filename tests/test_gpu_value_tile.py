"""The value role of the persistent FFN launch (csrc/lm_kernels.hip k_ffn_persist) at 17..32 rows: 16-row x
128-column tiles (gemm2_body kRoleFfnValue16 -- half the key-slab bytes staged per workgroup, two column
tiles per wave) against the 32-row x 64-column tiles they replace (forms = RWKVTTS_FORM_VALUE_TILE_32X64)
and against the separate LN2 / key / value launches (RWKVTTS_FORM_SEPARATE_FFN). Every output element
takes the same staging arithmetic and the same MFMA sequence, so everything must agree bit for bit: the
tokens, the logits the last step left on the device and the whole recurrent state (WKV state and both
token-shift vectors) of every slot. No tolerance.

Engines: the 0.4B widths (the persistent forms need C = 1024, F = 4096), two layers, random weights,
graph-replayed decode steps. A request decodes its 32 global tokens before the semantic ones, so a run is
32 + FIXED decode steps of R rows each (every request has the same prompt length and token count, so every
decode step has all R rows). Up to 16 rows launch_ffn_persist keeps the 32 x 64 role (the second row
group would be empty); those row counts are checked against the separate launches as well."""
import numpy as np
import pytest

import rwkvtts
from rwkvtts import weights as W
from helpers import make_request, synth_text

pytestmark = pytest.mark.gpu

_F = rwkvtts._ffi
FORMS = {"tile16": 0, "tile32": _F.FORM_VALUE_TILE_32X64, "separate": _F.FORM_SEPARATE_FFN}
FIXED = 7
HEAD_ROWS = 8193


@pytest.fixture(scope="module")
def blobs():
    return {"bf16": W.synth_blob(W.DIMS_MID, seed=20251205, dtype=_F.DTYPE_BF16),
            "f16": W.synth_blob(W.DIMS_MID, seed=7, dtype=_F.DTYPE_F16)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(blob, forms, rows, fixed=FIXED):
    """(tokens, logits of the last step [rows][HEAD_ROWS], recurrent states [rows][state floats])"""
    rt = rwkvtts.SharedRwkvRuntime(blob, max_slots=32, token_chunk_size=2048, use_graphs=True, forms=forms)
    try:
        assert rt.stats()["persistent"] == 1
        reqs = [make_request(synth_text(700 + i), seed=30 + i, fixed=fixed) for i in range(rows)]
        toks = rt.generate_batch(reqs)
        assert all(len(g) == 32 and len(s) == fixed for g, s in toks), [(len(g), len(s)) for g, s in toks]
        logits = rt.last_logits(rows, HEAD_ROWS)
        states = np.stack([rt.read_slot(s) for s in range(rows)])
        return toks, logits, states
    finally:
        rt.close()


def _assert_same(got, ref, what):
    assert got[0] == ref[0], (what, "tokens")
    for name, x, y in (("logits", got[1], ref[1]), ("state", got[2], ref[2])):
        bx, by = _bits(x), _bits(y)
        assert bx.shape == by.shape, (what, name)
        diff = np.argwhere(bx != by)
        assert diff.size == 0, (what, name, len(diff), diff[:4].tolist())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("rows", [17, 24, 31, 32])
def test_value_tile_16x128_bitwise(blobs, dtype, rows):
    ref = _run(blobs[dtype], FORMS["separate"], rows)
    assert np.isfinite(ref[1]).all()
    for form in ("tile16", "tile32"):
        _assert_same(_run(blobs[dtype], FORMS[form], rows), ref, (form, dtype, rows))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("rows", [1, 16])
def test_up_to_16_rows_keep_the_32x64_role(blobs, dtype, rows):
    """R <= 16: launch_ffn_persist picks the 32 x 64 role whatever the form bit says (R = 1: the row-fused
    granule form); the default forms, the form bit and the separate launches agree bit for bit."""
    ref = _run(blobs[dtype], FORMS["separate"], rows)
    for form in ("tile16", "tile32"):
        _assert_same(_run(blobs[dtype], FORMS[form], rows), ref, (form, dtype, rows))


def _hot_ffn_blob(dims, layer, factor):
    """tests/test_gpu_f16_range.py's construction: an f16 model whose layer-`layer` key weights are scaled
    so that relu(k)^2 leaves the f16 range"""
    blob = W.synth_blob(dims, seed=31, dtype=_F.DTYPE_F16)
    lay, _ = W.layout(dims)
    for (l, t, off, r, c, m) in lay:
        if l == layer and t == W.L_FFN_K:
            a = blob[off:off + r * c * 2].view(np.float16)
            a[:] = (a.astype(np.float32) * factor).astype(np.float16)
    return blob


def _layer0_key_max(blob, dims, prev_states, states):
    """max_j k_j of layer 0 in the last forwarded step of every row, recomputed in f32 from the recurrent
    states: the FFN token-shift slot of layer 0 holds LN2(h) of the last token forwarded, so with the
    states of a run one token shorter (the same token stream: the same seeds) the last step's FFN input
    is xk = x_t + (x_{t-1} - x_t) * ffn.x_k"""
    C, H = dims["n_embd"], dims["n_embd"] // 64
    lay, _ = W.layout(dims)
    ten = {t: (off, r, c) for (l, t, off, r, c, m) in lay if l == 0}
    off, r, c = ten[W.L_FFN_K]
    wk = blob[off:off + r * c * 2].view(np.float16).astype(np.float32).reshape(r, c)
    off, _, _ = ten[W.L_FFN_XK]
    mu = blob[off:off + C * 4].view(np.float32)
    o = C + H * 4096
    x, xp = states[:, o:o + C], prev_states[:, o:o + C]
    xk = x + (xp - x) * mu
    return (xk @ wk.T).max(axis=1)


def test_value_tile_f16_row_exponent_in_both_row_groups():
    """f16 relu^2 rows past 65504 (staged scaled by a power of two per row and K-slice, s_rexp) in rows
    0..15 and in rows 16..31, so both row groups of the 16 x 128 tile scale rows: bitwise the separate
    launches' and the 32 x 64 tile's."""
    dims = W.DIMS_MID
    blob = _hot_ffn_blob(dims, layer=0, factor=600.0)
    prev = _run(blob, FORMS["separate"], 32, fixed=FIXED - 1)
    ref = _run(blob, FORMS["separate"], 32)
    assert [(g, s[:FIXED - 1]) for g, s in ref[0]] == prev[0]  # one token more of the same streams
    assert np.isfinite(ref[1]).all()
    # k > 256 (k^2 > 65504) in the last decode step, in a row of each row group
    kmax = _layer0_key_max(blob, dims, prev[2], ref[2])
    print("layer-0 max k per row:", np.round(kmax).tolist())
    assert kmax[:16].max() > 256.0 * 1.05 and kmax[16:].max() > 256.0 * 1.05, kmax.tolist()
    for form in ("tile16", "tile32"):
        _assert_same(_run(blob, FORMS[form], 32), ref, (form, "hot f16"))
