"""MXFP6 (E2M3, E3M2) and MXINT8 weights (RWKVTTS_QUANT_MXFP6_E2M3 / MXFP6_E3M2 / MXINT8) on the GPU, by the
construction of tests/test_gpu_mx.py: the quantisation rule through rwkvtts_mx_roundtrip against
tests/mx_ref.py bit for bit, the GEMM (k_gemm_mx) through an unquantised engine on the dequantised blob.
tiny and c384 have the 128-deep K-slices (c384: key split 3), mid the 256-deep ones, split-K and the
tile-table launch; the 70-row step is past the 64-row switch (relu^2 planes)."""
import numpy as np
import pytest

import mx_ref
import rwkvtts
import test_gpu_mx as tgm
from rwkvtts import weights as W
from test_mx_ocp_cpu import OCP  # (its import adds the three formats to mx_ref.FORMATS)

pytestmark = pytest.mark.gpu

CASES = [("tiny", "mxfp6_e2m3", 2), ("c384", "mxfp6_e3m2", 2), ("mid", "mxint8", 1), ("mid", "mxfp6_e2m3", 1)]


def _int8_matrix():
    """tgm._roundtrip_matrix for MXINT8, whose 64 midpoints per binade do not fit one block: elements are
    i / 64, so every odd multiple of 2^-7 is a tie."""
    odd = lambda idx: [(2 * i + 1) / 128 for i in idx]
    sat = 127 / 64
    blocks = []
    for s in (1.0, 2.0 ** -20, 2.0 ** 90):
        # amax = 2^n: the ties below 2^-3 (negative), 8 around the middle, the 8 highest under the maximum
        blocks.append([s * x for x in [1.0] + [-x for x in odd(range(8))] + odd(range(28, 36)) + odd(range(56, 64))])
        # amax just below 2^(n + 1), itself past saturation: the 8 lowest ties of [1, 2), 8 between, the 8 highest
        blocks.append([s * x for x in [255 / 128] + [1 + x for x in odd(range(8)) + odd(range(28, 36)) + odd(range(56, 64))]])
        blocks.append([s * x for x in [255 / 128, -255 / 128, 253 / 128, sat, -sat, 1.0]])  # past saturation
    tiny = 2.0 ** -126
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


@pytest.mark.parametrize("fmt", list(OCP))
def test_roundtrip(fmt):
    w = _int8_matrix() if fmt == "mxint8" else tgm._roundtrip_matrix(fmt)
    got, want = rwkvtts.runtime.mx_roundtrip(fmt, w), mx_ref.dequantised(w, fmt)
    bad = np.argwhere(got != want)
    assert not len(bad), [(hex(w[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]]


@pytest.fixture(scope="module", params=CASES, ids=["-".join(map(str, c)) for c in CASES])
def pair(request):
    """tgm.pair for this module's cases"""
    name, fmt, ql = request.param
    dims = tgm.DIMS[name]
    blob = W.synth_blob(dims, seed=321)
    deq = mx_ref.dequantised_blob(blob, dims, fmt, ql)
    assert not np.array_equal(blob, deq)
    kw = dict(max_slots=4, token_chunk_size=128, use_graphs=True)
    rt_mx = rwkvtts.SharedRwkvRuntime(blob, quant_layers=ql, quant_type=fmt, **kw)
    rt_16 = rwkvtts.SharedRwkvRuntime(deq, **kw)
    yield dims, deq, rt_mx, rt_16
    rt_mx.close()
    rt_16.close()


def test_forward_bitwise(pair):
    tgm.test_forward_bitwise(pair)  # 70 tokens in one call, 35 + 35, four slots in one-token steps


def test_f16_refused():
    blob = W.synth_blob(W.DIMS_TINY, seed=1, dtype=rwkvtts._ffi.DTYPE_F16)
    with pytest.raises(rwkvtts._ffi.RwkvTtsError) as e:
        rwkvtts.SharedRwkvRuntime(blob, max_slots=2, quant_layers=1, quant_type="mxint8")
    assert e.value.code == rwkvtts._ffi.EUNSUPPORTED
